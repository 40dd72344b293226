// mrgs_shade.hip -- environment-cubemap mip lookup and deferred split-sum specular shading on gfx950; the fetch itself is mrgs_envmap.h.
//
//   envmap_lookup_{fwd,bwd}_kernel : EnvLight.__call__ (scene/light.py:99-129): roughness -> mip level (get_mip, :88-96),
//                                    seamless trilinear cubemap fetch over the mip chain, sigmoid.
//   shade_specular_fwd_kernel,       get_specular_color_surfel (utils/refl_utils.py:364-419) fused into one pass per pixel:
//   shade_fused_bwd_kernel<>       : camera ray (sample_camera_rays :54-73), mirror direction (reflection :95-98), split-sum
//                                    FG LUT fetch (:373-374), environment lookup (:376), Fresnel-style weight (:377),
//                                    specular = light * alpha * weight (:400-401); render_surfel's compositing rides in both.
//
// The reference does this with ~25 elementwise torch kernels plus two nvdiffrast `dr.texture` launches.
// Memory-bound by design: one pixel per lane, ~100 B/pixel in, 36 B/pixel out; the 1.6 MB mip chain and the 512 KB LUT stay
// in L2.  Texel gradients are accumulated with fp32 atomics (mirror directions of neighbouring pixels hit the same texels).
// Each group of kernels is followed by its entry points.
#include "mrgs_internal.h"
#include "mrgs_model_math.h"
#include "mrgs_envmap.h"

struct Map {   // strided [H,W,C] view
    const float* p;
    long long sh, sw, sc;
};

// ---- texel-gradient accumulation of the deferred shading backward ----------------------------------------------------------
// Measured on MI355X (tools/ubench/lds_atomic, tools/shade_stats.py): a scattered global float atomic costs the chip
// ~1/25 ns, an LDS float atomic (ds_add_f32) ~3 cycles PER ACTIVE LANE of its CU's LDS (200 G/s chip-wide; integer compare-and-swap is
// ten times faster), a VALU instruction 4 cycles per wave on one of four SIMDs -- so lanes are merged on the VALU first, then in LDS, and
// only what is left leaves the CU:
//   1. run_merge: neighbouring pixels mirror into the same texels in RUNS along a row (a 64 x 1 wave footprint touches ~9 distinct
//      texel footprints of a 64 x 64 level on the bench scene, 49 lanes using it): a segmented sum over runs of equal key inside each
//      16-lane row (four row_shr DPP steps) leaves one lane per run;
//   2. levels that fit the workgroup's LDS (coarsest first, MRGS_SHADE_LDS_FLOATS) accumulate in a dense LDS copy;
//   3. the finer levels go through a 4 096-entry LDS hash table (key = level | texel, CAS insert with linear probing, three float
//      accumulators per entry): a 64 x 12-pixel tile touches ~35 footprints of the 64 x 64 level, 590 pixels using it.  The table is
//      flushed with global atomics when half full (checked between tiles) and at the end; a lane that finds no slot in 8 probes adds
//      straight to global memory.
#define MRGS_SHADE_HASH_BITS 12
#define MRGS_SHADE_HASH_SIZE (1 << MRGS_SHADE_HASH_BITS)
#define MRGS_SHADE_KEY_NONE 0xffffffffu

// Sum v over the run of consecutive lanes (inside a 16-lane row) that hold the same key; true in the lane that ends a run, which then
// holds the run's total.  Hillis-Steele segmented scan: (v, head) o (v', head') = head' ? (v', 1) : (v + v', head).
__device__ __forceinline__ bool run_merge(unsigned key, float v[3])
{
#define SHR(x, n, old) __builtin_amdgcn_update_dpp((int)(old), (int)(x), 0x110 + (n), 0xf, 0xf, false)
    const unsigned prev = (unsigned)SHR(key, 1, ~key);                    // lane 0 of a row: no source -> old = ~key != key
    int head = prev != key;
    const int next_head = __builtin_amdgcn_update_dpp(1, head, 0x101, 0xf, 0xf, false);     // row_shl:1; lane 15 of a row: 1
#pragma unroll
    for (int d = 1; d <= 8; d <<= 1) {
        const float m = head ? 0.f : 1.f;
        float p0, p1, p2;
        int ph;
        if (d == 1) { p0 = __int_as_float(SHR(__float_as_int(v[0]), 1, 0)); p1 = __int_as_float(SHR(__float_as_int(v[1]), 1, 0)); p2 = __int_as_float(SHR(__float_as_int(v[2]), 1, 0)); ph = SHR(head, 1, 1); }
        else if (d == 2) { p0 = __int_as_float(SHR(__float_as_int(v[0]), 2, 0)); p1 = __int_as_float(SHR(__float_as_int(v[1]), 2, 0)); p2 = __int_as_float(SHR(__float_as_int(v[2]), 2, 0)); ph = SHR(head, 2, 1); }
        else if (d == 4) { p0 = __int_as_float(SHR(__float_as_int(v[0]), 4, 0)); p1 = __int_as_float(SHR(__float_as_int(v[1]), 4, 0)); p2 = __int_as_float(SHR(__float_as_int(v[2]), 4, 0)); ph = SHR(head, 4, 1); }
        else { p0 = __int_as_float(SHR(__float_as_int(v[0]), 8, 0)); p1 = __int_as_float(SHR(__float_as_int(v[1]), 8, 0)); p2 = __int_as_float(SHR(__float_as_int(v[2]), 8, 0)); ph = SHR(head, 8, 1); }
        v[0] = fmaf(p0, m, v[0]); v[1] = fmaf(p1, m, v[1]); v[2] = fmaf(p2, m, v[2]);
        head |= ph;
    }
#undef SHR
    return next_head != 0;
}

struct ShadeAcc {          // the workgroup's LDS accumulators
    float* dense;          // coarse levels, EnvMips::lds_off
    unsigned* keys;        // hash table of the finer levels
    float* vals;
    unsigned* count;       // entries taken so far (never reset: the kernel remembers its value at the last flush)
};

// one merged contribution (the lane ends a run; key = level << 24 | texel) into the workgroup's accumulators; loff = the level's
// offset in the dense LDS copy or < 0
__device__ __forceinline__ void acc_add(const EnvMips& m, const ShadeAcc& A, int lk, int loff, int idx, const float v[3])
{
    if (loff >= 0) {
        float* a = A.dense + loff + idx * 3;
        atomicAdd(a, v[0]); atomicAdd(a + 1, v[1]); atomicAdd(a + 2, v[2]);
        return;
    }
    const unsigned key = ((unsigned)lk << 24) | (unsigned)idx;
    unsigned h = (key * 2654435761u) >> (32 - MRGS_SHADE_HASH_BITS);
    int slot = -1;
    for (int p = 0; p < 8; ++p) {
        const unsigned old = atomicCAS(&A.keys[h], MRGS_SHADE_KEY_NONE, key);
        if (old == MRGS_SHADE_KEY_NONE) atomicAdd(A.count, 1u);
        if (old == MRGS_SHADE_KEY_NONE || old == key) { slot = (int)h; break; }
        h = (h + 1) & (MRGS_SHADE_HASH_SIZE - 1);
    }
    if (slot >= 0) {
        float* a = A.vals + slot * 3;
        atomicAdd(a, v[0]); atomicAdd(a + 1, v[1]); atomicAdd(a + 2, v[2]);
    } else {
        float* g = m.grad[lk] + (size_t)(blockIdx.x % (unsigned)m.copies[lk]) * (size_t)(6 * m.res[lk] * m.res[lk] * 3) + (size_t)idx * 3;
        atomicAdd(g, v[0]); atomicAdd(g + 1, v[1]); atomicAdd(g + 2, v[2]);
    }
}

// the eight taps of one pixel's fetch: merged along the row, then accumulated (wave-convergent: every lane of the wave calls it).
// grad_mask: bit l = level l takes gradients (scalar, built once per kernel: the per-lane level must not index the argument struct here)
__device__ __forceinline__ void env_scatter_tile(const EnvMips& m, unsigned grad_mask, const ShadeAcc& A, const EnvSample& s, const Taps tp[2],
                                                 const float gL[3])
{
    const bool any = gL[0] != 0.f || gL[1] != 0.f || gL[2] != 0.f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float wk = k == 0 ? 1.f - s.f : s.f;
        const int lk = k == 0 ? s.l0 : s.l1;
        const bool lev = any && wk != 0.f && ((grad_mask >> lk) & 1u);
        int loff = m.lds_off[0];
#pragma unroll
        for (int i = 1; i < MRGS_MAX_MIPS; i++) loff = (lk == i) ? m.lds_off[i] : loff;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float wq = wk * tp[k].w[q];
            float v[3] = {gL[0] * wq, gL[1] * wq, gL[2] * wq};
            const bool live = lev && tp[k].w[q] != 0.f;
            const unsigned key = live ? (((unsigned)lk << 24) | (unsigned)tp[k].idx[q]) : MRGS_SHADE_KEY_NONE;
            if (!live) { v[0] = 0.f; v[1] = 0.f; v[2] = 0.f; }
            const bool last = run_merge(key, v);
            if (last && key != MRGS_SHADE_KEY_NONE) acc_add(m, A, lk, loff, tp[k].idx[q], v);
        }
    }
}

// every entry of the hash table -> global memory, table emptied (all threads of the workgroup; barriers are the caller's)
__device__ __forceinline__ void acc_flush_hash(const EnvMips& m, const ShadeAcc& A, int nthreads)
{
    for (int i = threadIdx.x; i < MRGS_SHADE_HASH_SIZE; i += nthreads) {
        const unsigned key = A.keys[i];
        if (key == MRGS_SHADE_KEY_NONE) continue;
        const int lk = (int)(key >> 24), idx = (int)(key & 0xffffffu);
        float* g = m.grad[lk] + (size_t)(blockIdx.x % (unsigned)m.copies[lk]) * (size_t)(6 * m.res[lk] * m.res[lk] * 3) + (size_t)idx * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = A.vals[i * 3 + c];
            if (v != 0.f) atomicAdd(g + c, v);
            A.vals[i * 3 + c] = 0.f;
        }
        A.keys[i] = MRGS_SHADE_KEY_NONE;
    }
}

// ---- standalone environment lookup ---------------------------------------------------------------------
__global__ void __launch_bounds__(256) envmap_lookup_fwd_kernel(EnvMips m, long long N, const float* __restrict__ dirs,
                                                                const float* __restrict__ roughness, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const f3 d = mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    const FaceUV fu = dir_to_face(d);
    float dl;
    const bool use_mips = roughness != nullptr;
    const float level = use_mips ? mip_level(m, roughness[i], dl) : 0.f;
    EnvSample s;
    Taps tp[2];
    env_fetch(m, fu, level, use_mips, s, tp);
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * i + c] = sigmoid_fast(s.L[c]);
}

__global__ void __launch_bounds__(256) envmap_lookup_bwd_kernel(EnvMips m, long long N, const float* __restrict__ dirs,
                                                                const float* __restrict__ roughness, const float* __restrict__ g_out,
                                                                float* __restrict__ g_dirs, float* __restrict__ g_rough)
{
    const long long i_ = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i_ < N;              // out-of-range lanes stay alive (the texel scatter is wave-convergent)
    const long long i = valid ? i_ : N - 1;
    const f3 d = mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    const FaceUV fu = dir_to_face(d);
    float dl = 0.f;
    const bool use_mips = roughness != nullptr;
    const float level = use_mips ? mip_level(m, roughness[i], dl) : 0.f;
    EnvSample s;
    Taps tp[2];
    env_fetch(m, fu, level, use_mips, s, tp);
    float gL[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float y = sigmoid_fast(s.L[c]);
        gL[c] = valid ? g_out[3 * i + c] * y * (1.f - y) : 0.f;
    }
    f3 gd;
    float glev;
    env_fetch_bwd<true>(m, fu, d, s, tp, gL, gd, glev);
    if (valid && g_dirs) { g_dirs[3 * i] = gd.x; g_dirs[3 * i + 1] = gd.y; g_dirs[3 * i + 2] = gd.z; }
    if (valid && g_rough) g_rough[i] = use_mips ? glev * dl : 0.f;
}

extern "C" int mrgs_envmap_lookup_forward(const MrgsEnvMips* mips, int64_t N, const float* dirs, const float* roughness, float* out, void* stream)
{
    EnvMips m;
    if (int rc = make_mips(mips, m)) return rc;
    if (N < 0 || (N > 0 && (!dirs || !out))) return MRGS_E_BAD_ARG;
    if (N == 0) return MRGS_OK;
    hipLaunchKernelGGL(envmap_lookup_fwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, (long long)N, dirs,
                       roughness, out);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_envmap_lookup_backward(const MrgsEnvMips* mips, int64_t N, const float* dirs, const float* roughness, const float* g_out,
                                           float* g_dirs, float* g_roughness, void* stream)
{
    EnvMips m;
    if (int rc = make_mips(mips, m)) return rc;
    if (N < 0 || (N > 0 && (!dirs || !g_out))) return MRGS_E_BAD_ARG;
    if (N == 0) return MRGS_OK;
    hipLaunchKernelGGL(envmap_lookup_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, (long long)N, dirs,
                       roughness, g_out, g_dirs, g_roughness);
    return MRGS_LAUNCH_STATUS();
}

// ---- fused deferred specular shading ---------------------------------------------------------------------
struct ShadeCam { float Kinv[9]; const float* R; const float* T; };   // R: Camera.R (c2w rotation, [3,3]); T: w2c translation

struct ShadePix {
    f3 wo, n, r, rn;
    float ndv, rlen, u, v, rough, refl, alpha;
    float albedo[3], fg[2], dfg_du[2], dfg_dv[2];
    bool u_in, v_in;
};


// the camera of a launch in scalar registers: K^-1, Camera.R (c2w rotation), the w2c translation and the camera centre -R T
struct ShadeCamS { float Kinv[9], R[9], t[3], ro[3]; };
__device__ __forceinline__ float sreg(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ ShadeCamS shade_cam_load(const ShadeCam& cam)
{
    ShadeCamS c;
#pragma unroll
    for (int i = 0; i < 9; i++) { c.Kinv[i] = cam.Kinv[i]; c.R[i] = sreg(cam.R[i]); }
#pragma unroll
    for (int i = 0; i < 3; i++) c.t[i] = sreg(cam.T[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) c.ro[i] = -(c.R[3 * i] * c.t[0] + c.R[3 * i + 1] * c.t[1] + c.R[3 * i + 2] * c.t[2]);
    return c;
}

// the per-pixel inputs of the shading, fetched in one go (nine independent loads in flight)
struct ShadeIn { float n[3], rough, refl, alpha, albedo[3]; };
__device__ __forceinline__ ShadeIn shade_load(int x, int y, const Map& albedo, const Map& normal, const Map& alpha, const Map& refl, const Map& rough)
{
    ShadeIn in;
    const long long o = (long long)y * normal.sh + (long long)x * normal.sw;
    in.n[0] = normal.p[o]; in.n[1] = normal.p[o + normal.sc]; in.n[2] = normal.p[o + 2 * normal.sc];
    in.rough = rough.p[(long long)y * rough.sh + (long long)x * rough.sw];
    in.refl = refl.p[(long long)y * refl.sh + (long long)x * refl.sw];
    in.alpha = alpha.p[(long long)y * alpha.sh + (long long)x * alpha.sw];
    const long long oa = (long long)y * albedo.sh + (long long)x * albedo.sw;
#pragma unroll
    for (int c = 0; c < 3; c++) in.albedo[c] = albedo.p[oa + c * albedo.sc];
    return in;
}

// w_o of a pixel: sample_camera_rays (utils/refl_utils.py:54-73), pixel centres at integer coordinates
__device__ __forceinline__ f3 shade_view_dir(const ShadeCamS& cam, int x, int y)
{
    const float fx_ = (float)x, fy_ = (float)y;
    const f3 pc = mk(cam.Kinv[0] * fx_ + cam.Kinv[1] * fy_ + cam.Kinv[2], cam.Kinv[3] * fx_ + cam.Kinv[4] * fy_ + cam.Kinv[5],
                     cam.Kinv[6] * fx_ + cam.Kinv[7] * fy_ + cam.Kinv[8]);
    // Camera.R is stored transposed (c2w); the reference re-transposes it: world = (pc - T) @ R^T^T ... = c2w * (pc - T)
    const float* R = cam.R;
    const f3 q = mk(pc.x - cam.t[0], pc.y - cam.t[1], pc.z - cam.t[2]);
    const f3 pw = mk(R[0] * q.x + R[1] * q.y + R[2] * q.z, R[3] * q.x + R[4] * q.y + R[5] * q.z, R[6] * q.x + R[7] * q.y + R[8] * q.z);
    f3 rd = mk(pw.x - cam.ro[0], pw.y - cam.ro[1], pw.z - cam.ro[2]);
    const float inv = __builtin_amdgcn_rsqf(dot3(rd, rd));
    rd = mk(rd.x * inv, rd.y * inv, rd.z * inv);
    return mk(-rd.x, -rd.y, -rd.z);
}

__device__ __forceinline__ void shade_setup(const ShadeCamS& cam, int x, int y, const ShadeIn& in, const float* __restrict__ lut, int lres, ShadePix& p)
{
    p.wo = shade_view_dir(cam, x, y);
    p.n = mk(in.n[0], in.n[1], in.n[2]);
    p.ndv = dot3(p.wo, p.n);                                    // reflection(), :95-98
    p.r = mk(2.f * p.n.x * p.ndv - p.wo.x, 2.f * p.n.y * p.ndv - p.wo.y, 2.f * p.n.z * p.ndv - p.wo.z);
    p.rlen = fmaxf(__builtin_amdgcn_sqrtf(dot3(p.r, p.r)), 1e-20f);              // safe_normalize
    const float irl = shade_rcp(p.rlen);
    p.rn = mk(p.r.x * irl, p.r.y * irl, p.r.z * irl);
    p.rough = in.rough;
    p.refl = in.refl;
    p.alpha = in.alpha;
#pragma unroll
    for (int c = 0; c < 3; c++) p.albedo[c] = in.albedo[c];
    p.u_in = p.ndv >= 0.f && p.ndv <= 1.f;
    p.v_in = p.rough >= 0.f && p.rough <= 1.f;
    p.u = fminf(fmaxf(p.ndv, 0.f), 1.f);
    p.v = fminf(fmaxf(p.rough, 0.f), 1.f);
    lut_fetch(lut, lres, p.u, p.v, p.fg, p.dfg_du, p.dfg_dv);
}

__global__ void __launch_bounds__(256) shade_specular_fwd_kernel(EnvMips m, ShadeCam cam, int H, int W, Map albedo, Map normal, Map alpha,
                                                                 Map refl, Map rough, const float* __restrict__ lut, int lres,
                                                                 float* __restrict__ specular /*[3,H,W]*/, float* __restrict__ direct /*[3,H,W]*/,
                                                                 float* __restrict__ weight /*[H,W,3]*/,
                                                                 // render_surfel's compositing in the same pass (render != nullptr; mrgs_surfel_composite_forward)
                                                                 const float* __restrict__ base /*[3,H,W]*/, const float* __restrict__ bg, int srgb,
                                                                 float* __restrict__ render /*[3,H,W]*/, float* __restrict__ diffuse /*[3,H,W]*/,
                                                                 float* __restrict__ zero_fill, long long zero_floats)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    {   // side job for the backward of this very render: clear the texel-gradient buffers its shading backward accumulates into (a fill
        // launch of its own otherwise: the backward's first kernel is the one that accumulates)
        const long long tid = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x, nthr = (long long)gridDim.x * gridDim.y * 256;
        for (long long i = tid; i < zero_floats; i += nthr) zero_fill[i] = 0.0f;
    }
    if (x >= W || y >= H) return;
    const ShadeCamS cs = shade_cam_load(cam);
    const ShadeIn in = shade_load(x, y, albedo, normal, alpha, refl, rough);
    ShadePix p;
    shade_setup(cs, x, y, in, lut, lres, p);
    const FaceUV fu = dir_to_face(p.rn);
    float dl;
    const float level = mip_level(m, p.rough, dl);
    EnvSample s;
    Taps tp[2];
    env_fetch(m, fu, level, true, s, tp);
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float light = sigmoid_fast(s.L[c]);
        const float wgt = (0.04f * (1.f - p.refl) + p.albedo[c] * p.refl) * p.fg[0] + p.fg[1];
        direct[c * HW + pix] = light;
        weight[pix * 3 + c] = wgt;
        const float spec = light * p.alpha * wgt;
        specular[c * HW + pix] = spec;
        if (render != nullptr) {     // diffuse = (1 - refl) base, render = [srgb](diffuse + specular) + bg (1 - alpha)  (gaussian_renderer/__init__.py:436-445)
            const float d = (1.0f - p.refl) * base[c * HW + pix];
            float v = d + spec;
            if (srgb) v = lin2srgb(v);
            render[c * HW + pix] = v + bg[c] * (1.0f - p.alpha);
            diffuse[c * HW + pix] = d;
        }
    }
}

// ---- backward of the deferred shading -----------------------------------------------------------------------------------------
// Persistent workgroups (one per CU, 12 waves): each keeps an LDS copy of the texel gradients of the coarse mip levels
// (<= MRGS_SHADE_LDS_FLOATS floats: 32x32 and 16x16 cubemap levels = 90 KB) and a hash table for the finer ones (64 KB), walks
// 64x12-pixel tiles of the image and flushes both at the end (see "texel-gradient accumulation" above).  COMPOSITE: render_surfel's
// compositing backward (gaussian_renderer/__init__.py:436-445) in front of the shading's, in the same lane: its shares of g_specular,
// g_refl and g_alpha never leave registers (rounds 2-5 ran it as a launch of its own, 10.7 us for 36 bytes a pixel each way).
// Round 6 measured the alternative the register count suggests (168 VGPRs, a dozen spilled, three waves per SIMD) -- a per-pixel launch
// without LDS (134 VGPRs, no spill) that leaves the pixel's d loss / d sample in a scratch map, and a scatter launch that recomputes the
// taps (72 VGPRs): 35 + 45 us against this kernel's 69.  The scatter launch alone is 11 us of loop, loads, accumulator set-up and flush,
// + 10 of recomputed taps, + 4 of run merging, + 20 of LDS float atomics and hash probes (8 with integer atomics): the persistent
// form hides the accumulation's latency behind the fetch of the next pixel, the split form pays both in turn.  Dropped.
#define MRGS_SHADE_LDS_FLOATS 23552
#ifndef MRGS_SHADE_FUSED_THREADS
#define MRGS_SHADE_FUSED_THREADS 768
#endif
template <bool COMPOSITE>
__global__ void __launch_bounds__(MRGS_SHADE_FUSED_THREADS) shade_fused_bwd_kernel(
    EnvMips m, ShadeCam cam, int H, int W, Map albedo, Map normal, Map alpha, Map refl, Map rough, const float* __restrict__ lut, int lres,
    const float* __restrict__ g_specular, const float* __restrict__ g_direct, const float* __restrict__ g_weight,
    float* __restrict__ g_albedo /*[H,W,3]*/, float* __restrict__ g_normal /*[H,W,3]*/, float* __restrict__ g_alpha /*[H,W]*/,
    float* __restrict__ g_refl /*[H,W]*/, float* __restrict__ g_rough /*[H,W]*/, int tiles_x, int ntiles, int lds_floats,
    float* __restrict__ g_features, const float* __restrict__ g_refl_composite, const float* __restrict__ g_alpha_composite,
    int srgb, const float* __restrict__ base, const float* __restrict__ spec_fwd, const float* __restrict__ bg,
    const float* __restrict__ g_render, const float* __restrict__ g_diffuse, float* __restrict__ g_base)
{
    __shared__ float s_grad[MRGS_SHADE_LDS_FLOATS];
    __shared__ unsigned s_keys[MRGS_SHADE_HASH_SIZE];
    __shared__ float s_vals[MRGS_SHADE_HASH_SIZE * 3];
    __shared__ unsigned s_count;
    for (int i = threadIdx.x; i < lds_floats; i += MRGS_SHADE_FUSED_THREADS) s_grad[i] = 0.f;
    for (int i = threadIdx.x; i < MRGS_SHADE_HASH_SIZE; i += MRGS_SHADE_FUSED_THREADS) { s_keys[i] = MRGS_SHADE_KEY_NONE; s_vals[3 * i] = 0.f; s_vals[3 * i + 1] = 0.f; s_vals[3 * i + 2] = 0.f; }
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const ShadeAcc A = {s_grad, s_keys, s_vals, &s_count};
    const size_t HW = (size_t)H * W;
    unsigned flushed_at = 0u;                              // value of the (never reset) entry counter at the last flush
    int since_check = 0;
    const ShadeCamS cs = shade_cam_load(cam);
    unsigned grad_mask = 0u;
#pragma unroll
    for (int i = 0; i < MRGS_MAX_MIPS; i++) grad_mask |= (i < m.n && m.grad[i] != nullptr) ? (1u << i) : 0u;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x_ = (t % tiles_x) * 64 + (threadIdx.x & 63), y_ = (t / tiles_x) * (MRGS_SHADE_FUSED_THREADS / 64) + (threadIdx.x >> 6);
        const bool valid = x_ < W && y_ < H;    // out-of-image lanes stay alive (the texel scatter is wave-convergent)
        const int x = min(x_, W - 1), y = min(y_, H - 1);
        const size_t pix = (size_t)y * W + x;
        // every input of the pixel first: the maps and the upstream gradients are independent loads
        const ShadeIn in = shade_load(x, y, albedo, normal, alpha, refl, rough);
        float gs_[3], gd_[3], gw_[3];
        float g_refl_c = 0.f, g_alpha_c = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            gs_[c] = (valid && g_specular) ? g_specular[c * HW + pix] : 0.f;
            gd_[c] = (valid && g_direct) ? g_direct[c * HW + pix] : 0.f;
            gw_[c] = (valid && g_weight) ? g_weight[pix * 3 + c] : 0.f;
        }
        if constexpr (COMPOSITE) {
            // render = [srgb](k base + specular) + bg (1 - alpha), diffuse = k base, k = 1 - refl   (gaussian_renderer/__init__.py:436-445)
            const float k = 1.0f - in.refl;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float b = base[c * HW + pix];
                const float gR = (valid && g_render != nullptr) ? g_render[c * HW + pix] : 0.0f;
                g_alpha_c -= bg[c] * gR;
                float gl = gR;
                if (srgb) gl *= lin2srgb_grad(k * b + spec_fwd[c * HW + pix]);
                const float gd = gl + ((valid && g_diffuse != nullptr) ? g_diffuse[c * HW + pix] : 0.0f);
                if (valid) g_base[c * HW + pix] = k * gd;
                g_refl_c -= b * gd;
                gs_[c] += gl;
            }
        } else if (g_features != nullptr) {     // unreachable: no entry point launches the <false> instance with g_features any more
            g_refl_c = g_refl_composite[pix];
            g_alpha_c = g_alpha_composite[pix];
        }
        ShadePix p;
        shade_setup(cs, x, y, in, lut, lres, p);
        const FaceUV fu = dir_to_face(p.rn);
        float dl;
        const float level = mip_level(m, p.rough, dl);
        EnvSample s;
        Taps tp[2];
        env_fetch(m, fu, level, true, s, tp);
        float gL[3], ga = 0.f, gm = 0.f, gfg0 = 0.f, gfg1 = 0.f, galb[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float light = sigmoid_fast(s.L[c]);
            const float basec = 0.04f * (1.f - p.refl) + p.albedo[c] * p.refl;
            const float wgt = basec * p.fg[0] + p.fg[1];
            const float gs = gs_[c];
            const float gd = gd_[c] + gs * p.alpha * wgt;
            const float gw = gw_[c] + gs * light * p.alpha;
            ga += gs * light * wgt;
            gL[c] = gd * light * (1.f - light);
            galb[c] = gw * p.refl * p.fg[0];
            gm += gw * (p.albedo[c] - 0.04f) * p.fg[0];
            gfg0 += gw * basec;
            gfg1 += gw;
        }
        f3 g_rn;
        float g_level;
        env_fetch_bwd<false>(m, fu, p.rn, s, tp, gL, g_rn, g_level);
        // safe_normalize backward (the 1e-20 clamp never binds for finite normals)
        const float rg = dot3(p.rn, g_rn);
        const float irl = shade_rcp(p.rlen);
        const f3 g_r = mk((g_rn.x - p.rn.x * rg) * irl, (g_rn.y - p.rn.y * rg) * irl, (g_rn.z - p.rn.z * rg) * irl);
        // r = 2 n (n.wo) - wo ; NdotV = n.wo feeds the LUT's u coordinate
        const float g_ndv = p.u_in ? gfg0 * p.dfg_du[0] + gfg1 * p.dfg_du[1] : 0.f;
        const float grn = dot3(g_r, p.n);
        const f3 gn = mk(2.f * p.ndv * g_r.x + (2.f * grn + g_ndv) * p.wo.x, 2.f * p.ndv * g_r.y + (2.f * grn + g_ndv) * p.wo.y,
                         2.f * p.ndv * g_r.z + (2.f * grn + g_ndv) * p.wo.z);
        const float g_rough_v = (p.v_in ? gfg0 * p.dfg_dv[0] + gfg1 * p.dfg_dv[1] : 0.f) + g_level * dl;
        if (valid) {
            g_normal[pix * 3] = gn.x; g_normal[pix * 3 + 1] = gn.y; g_normal[pix * 3 + 2] = gn.z;
            if (g_features != nullptr) {
                g_alpha[pix] = g_alpha_c + ga;
                g_features[pix] = g_refl_c + gm;
                g_features[HW + pix] = g_rough_v;
#pragma unroll
                for (int c = 0; c < 3; c++) { g_features[(2 + c) * HW + pix] = galb[c]; g_features[(5 + c) * HW + pix] = 0.0f; }
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) g_albedo[pix * 3 + c] = galb[c];
                g_alpha[pix] = ga;
                g_refl[pix] = gm;
                g_rough[pix] = g_rough_v;
            }
        }
        if (!valid) { gL[0] = 0.f; gL[1] = 0.f; gL[2] = 0.f; }
        // (a wave of pixels that saw no environment light -- background: alpha = 0 makes gL an exact zero -- has nothing to add)
        if (grad_mask != 0u && __builtin_amdgcn_ballot_w64(gL[0] != 0.f || gL[1] != 0.f || gL[2] != 0.f) != 0ull)
            env_scatter_tile(m, grad_mask, A, s, tp, gL);
        // between tiles: a hash table more than half full goes out
        if (++since_check < 4) continue;
        since_check = 0;
        __syncthreads();
        const unsigned taken = s_count;                    // same value in every thread: entries are only taken before the barrier above
        if (taken - flushed_at > MRGS_SHADE_HASH_SIZE / 2) {
            acc_flush_hash(m, A, MRGS_SHADE_FUSED_THREADS);
            flushed_at = taken;
        }
        __syncthreads();
    }
    // flush: the hash table, then the LDS-resident levels into one of the level's global copies (untouched texels are skipped)
    __syncthreads();                 // every wave has left the tile loop (the loop only meets at a barrier every fourth tile)
    acc_flush_hash(m, A, MRGS_SHADE_FUSED_THREADS);
    for (int l = 0; l < m.n; l++) {
        if (m.lds_off[l] < 0 || m.grad[l] == nullptr) continue;
        const int n = 6 * m.res[l] * m.res[l] * 3;
        float* dst = m.grad[l] + (size_t)(blockIdx.x % (unsigned)m.copies[l]) * (size_t)n;
        for (int i = threadIdx.x; i < n; i += MRGS_SHADE_FUSED_THREADS) {
            const float v = s_grad[m.lds_off[l] + i];
            if (v != 0.f) atomicAdd(dst + i, v);
        }
    }
}

// ---- entry points of the deferred shading -----------------------------------------------------------------------------------
static Map to_map(const MrgsStridedMap& s) { Map r = {s.ptr, s.stride_h, s.stride_w, s.stride_c}; return r; }
static ShadeCam to_cam(const MrgsShadeFrame* fr)
{
    ShadeCam cam;
    for (int i = 0; i < 9; i++) cam.Kinv[i] = fr->Kinv[i];
    cam.R = fr->R; cam.T = fr->T;
    return cam;
}

extern "C" {

static int shade_specular_forward_impl(const MrgsEnvMips* mips, const MrgsShadeFrame* fr, float* specular, float* direct_light, float* specular_weight,
                                       const float* base_color, const float* bg, int srgb, float* render, float* diffuse, float* zero_fill,
                                       int64_t zero_floats, void* stream)
{
    EnvMips m;
    if (int rc = make_mips(mips, m)) return rc;
    if (!fr || fr->H <= 0 || fr->W <= 0 || !fr->R || !fr->T || !fr->lut || fr->lut_res < 1 || !specular || !direct_light || !specular_weight)
        return MRGS_E_BAD_ARG;
    if (zero_floats < 0 || (zero_floats > 0 && !zero_fill)) return MRGS_E_BAD_ARG;
    const dim3 grid((fr->W + 63) / 64, (fr->H + 3) / 4), block(256);
    hipLaunchKernelGGL(shade_specular_fwd_kernel, grid, block, 0, (hipStream_t)stream, m, to_cam(fr), fr->H, fr->W, to_map(fr->albedo), to_map(fr->normal),
                       to_map(fr->alpha), to_map(fr->refl), to_map(fr->roughness), fr->lut, fr->lut_res, specular, direct_light, specular_weight,
                       base_color, bg, srgb, render, diffuse, zero_fill, (long long)zero_floats);
    return MRGS_LAUNCH_STATUS();
}

int mrgs_shade_specular_forward(const MrgsEnvMips* mips, const MrgsShadeFrame* fr, float* specular, float* direct_light, float* specular_weight,
                                void* stream)
{
    return shade_specular_forward_impl(mips, fr, specular, direct_light, specular_weight, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, stream);
}

int mrgs_shade_specular_forward_composite(const MrgsEnvMips* mips, const MrgsShadeFrame* fr, const float* base_color, const float* bg, int32_t srgb,
                                          float* specular, float* direct_light, float* specular_weight, float* render, float* diffuse,
                                          float* zero_fill, int64_t zero_floats, void* stream)
{
    if (!base_color || !bg || !render || !diffuse) return MRGS_E_BAD_ARG;
    return shade_specular_forward_impl(mips, fr, specular, direct_light, specular_weight, base_color, bg, srgb ? 1 : 0, render, diffuse, zero_fill,
                                       zero_floats, stream);
}

// composite != nullptr: render_surfel's compositing backward in the same launch (mrgs_surfel_shade_composite_backward)
struct ShadeCompositeArgs { int srgb; const float *base, *spec_fwd, *bg, *g_render, *g_diffuse; float* g_base; };

static int shade_specular_backward_impl(const MrgsEnvMips* mips, const MrgsShadeFrame* fr, const float* g_specular, const float* g_direct_light,
                                        const float* g_specular_weight, float* g_albedo, float* g_normal, float* g_alpha, float* g_refl,
                                        float* g_roughness, float* g_features, const ShadeCompositeArgs* composite, void* stream)
{
    EnvMips m;
    if (int rc = make_mips(mips, m)) return rc;
    if (!fr || fr->H <= 0 || fr->W <= 0 || !fr->R || !fr->T || !fr->lut || !g_normal || !g_alpha) return MRGS_E_BAD_ARG;
    if (composite ? (!g_features || !composite->base || !composite->spec_fwd || !composite->bg || !composite->g_base)
                  : (!g_albedo || !g_refl || !g_roughness)) return MRGS_E_BAD_ARG;
    // the scatter keys pack (level << 24 | texel index): a level with 6 res^2 >= 2^24 texels (res >= 1673) would alias into the level bits
    for (int l = 0; l < m.n; l++)
        if (m.grad[l] != nullptr && 6ll * m.res[l] * m.res[l] >= (1ll << 24)) return MRGS_E_UNSUPPORTED;
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n_cu = v;
        else n_cu = 256;
    }
    // LDS-resident levels: from the coarsest up while they fit
    int lds_floats = 0;
    for (int l = m.n - 1; l >= 0; l--) {
        const int n = 6 * m.res[l] * m.res[l] * 3;
        if (m.grad[l] == nullptr || lds_floats + n > MRGS_SHADE_LDS_FLOATS) break;
        m.lds_off[l] = lds_floats;
        lds_floats += n;
    }
    const int rows = MRGS_SHADE_FUSED_THREADS / 64;
    const int tiles_x = (fr->W + 63) / 64, ntiles = tiles_x * ((fr->H + rows - 1) / rows);
    const dim3 grid(ntiles < n_cu ? ntiles : n_cu), block(MRGS_SHADE_FUSED_THREADS);
    // the two instances take the same arguments; the plain one gets the compositing's as zeros
    const ShadeCompositeArgs ca = composite ? *composite : ShadeCompositeArgs{};
    const auto kernel = composite ? shade_fused_bwd_kernel<true> : shade_fused_bwd_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, m, to_cam(fr), fr->H, fr->W, to_map(fr->albedo), to_map(fr->normal),
                       to_map(fr->alpha), to_map(fr->refl), to_map(fr->roughness), fr->lut, fr->lut_res, g_specular, g_direct_light, g_specular_weight,
                       g_albedo, g_normal, g_alpha, g_refl, g_roughness, tiles_x, ntiles, lds_floats, g_features, (const float*)nullptr, (const float*)nullptr,
                       ca.srgb, ca.base, ca.spec_fwd, ca.bg, ca.g_render, ca.g_diffuse, ca.g_base);
    return MRGS_LAUNCH_STATUS();
}

int mrgs_shade_specular_backward(const MrgsEnvMips* mips, const MrgsShadeFrame* fr, const float* g_specular, const float* g_direct_light,
                                 const float* g_specular_weight, float* g_albedo, float* g_normal, float* g_alpha, float* g_refl,
                                 float* g_roughness, void* stream)
{
    return shade_specular_backward_impl(mips, fr, g_specular, g_direct_light, g_specular_weight, g_albedo, g_normal, g_alpha, g_refl, g_roughness,
                                        nullptr, nullptr, stream);
}

int mrgs_surfel_shade_composite_backward(const MrgsEnvMips* mips, const MrgsShadeFrame* fr, int32_t srgb, const float* base_color, const float* specular,
                                         const float* bg, const float* g_render, const float* g_diffuse, const float* g_specular_extra,
                                         const float* g_direct_light, const float* g_specular_weight, float* g_base, float* g_normal, float* g_features,
                                         float* g_alpha, void* stream)
{
    if (!g_features) return MRGS_E_BAD_ARG;
    const ShadeCompositeArgs ca = {srgb, base_color, specular, bg, g_render, g_diffuse, g_base};
    return shade_specular_backward_impl(mips, fr, g_specular_extra, g_direct_light, g_specular_weight, nullptr, g_normal, g_alpha, nullptr, nullptr,
                                        g_features, &ca, stream);
}

}   // extern "C"
