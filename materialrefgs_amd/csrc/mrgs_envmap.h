// mrgs_envmap.h -- the environment cubemap as the kernel files see it: cube addressing, the seamless trilinear mip fetch and its adjoint,
// the split-sum FG LUT fetch, and the host-side translation of MrgsEnvMips.  What more than one of mrgs_shade.hip (lookup, deferred
// shading), mrgs_prefilter.hip (filters, mips) and mrgs_bounce.hip (one-bounce light) uses lives here once.
//
// The reference samples with two nvdiffrast `dr.texture` launches.  nvdiffrast is not vendored (requirements.txt:57 pins a local path), so
// its sampling rules are RESTATED here and in oracle/shading_oracle.py: texel centres at (i + 0.5) / res, bilinear taps, `clamp` boundary
// for the 2D LUT, seamless cube edges (a tap that falls off a face is taken from the face across the edge; the non-existent corner tap
// gets zero weight and the other three are renormalised), mip level = mip_level_bias clamped to [0, levels-1] with linear interpolation
// between the two nearest levels.  Face/orientation convention: cube_to_dir (scene/light_utils.py:24-31).
// tests/test_envmap_seams.py holds the restatement to the geometry of a cube and the kernels to the restatement.  PINNED BY GEOMETRY:
// the face orientation, all 12 seams, all 8 vertices, the weight sums, the level shares, the tangency of the direction gradient and
// that it is the slope of the forward inside a cell.  STILL A RESTATEMENT of nvdiffrast: the drop-and-renormalise rule of a vertex
// cell and its gradient with the renormalisation held constant.
// The quotients of the fetch are v_rcp_f32, 1 ulp, not IEEE: the note at shade_rcp below says why and which kernels keep the IEEE
// quotient.
#pragma once
#include "mrgs_internal.h"
#include "mrgs_wave.h"

struct EnvMips {   // by-value kernel argument
    int n;
    int res[MRGS_MAX_MIPS];
    const float* tex[MRGS_MAX_MIPS];
    float* grad[MRGS_MAX_MIPS];
    int copies[MRGS_MAX_MIPS];
    int lds_off[MRGS_MAX_MIPS];   // backward of the deferred shading: float offset of the level's LDS accumulator, -1 = global only
    float min_roughness, max_roughness;
};

// v_rcp_f32 (1 ulp) instead of the IEEE quotient (ten instructions and two mode switches each): the lookups and the split-sum shading are
// compared to 2e-5 of a map's range and their sampling rule is a restatement to begin with (header); the filter-building kernels of
// mrgs_prefilter.hip, which restate the reference's weights operation for operation, keep the IEEE quotient.  Every kernel of a fetch (a
// forward, and the backward that recomputes it) goes through the same inline functions, so the two agree on a pixel's taps.
__device__ __forceinline__ float shade_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float x, float y, float z) { f3 r = {x, y, z}; return r; }
__device__ __forceinline__ float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// direction -> (face, u, v) with u,v in [-1,1]; inverse of cube_to_dir (scene/light_utils.py:24-31)
struct FaceUV { int face; float u, v, inv_ma; int axis; float sgn; };
__device__ __forceinline__ FaceUV dir_to_face(f3 d)
{   // branch-free (selects): the callers inline it up to eight times per pixel
    FaceUV r;
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const bool mx = ax >= ay && ax >= az, my = !mx && ay >= az;
    const float ma = mx ? ax : (my ? ay : az), mc = mx ? d.x : (my ? d.y : d.z);
    const bool pos = mc >= 0.f;
    r.axis = mx ? 0 : (my ? 1 : 2);
    r.sgn = pos ? 1.f : -1.f;
    r.inv_ma = shade_rcp(ma);
    r.face = 2 * r.axis + (pos ? 0 : 1);
    // x-major: u = -+z, v = -y; y-major: u = x, v = +-z; z-major: u = +-x, v = -y
    const float un = mx ? (pos ? -d.z : d.z) : (my ? d.x : (pos ? d.x : -d.x));
    const float vn = my ? (pos ? d.z : -d.z) : -d.y;
    r.u = un * r.inv_ma;
    r.v = vn * r.inv_ma;
    return r;
}
__device__ __forceinline__ f3 face_to_dir(int s, float x, float y)
{
    switch (s) {
    case 0: return mk(1.f, -y, -x);
    case 1: return mk(-1.f, -y, x);
    case 2: return mk(x, 1.f, y);
    case 3: return mk(x, -1.f, -y);
    case 4: return mk(x, -y, 1.f);
    default: return mk(-x, -y, -1.f);
    }
}

// the four bilinear taps of one mip level: linear texel indices (face*res*res + y*res + x) and weights
struct Taps { int idx[4]; float w[4]; float wx, wy, norm; bool corner; };
__device__ __forceinline__ int wrap_tap(int face, int x, int y, int res)
{
    if (x >= 0 && x < res && y >= 0 && y < res) return (face * res + y) * res + x;
    // texel centre of the tap in the face's plane; the overshooting coordinate is pulled just across the edge so that the
    // re-projection lands on the border texel of the adjacent face with the edge-parallel coordinate unchanged
    const float eps = 1.0f / 4096.0f;
    float u = ((float)x + 0.5f) / (float)res * 2.0f - 1.0f;
    float v = ((float)y + 0.5f) / (float)res * 2.0f - 1.0f;
    if (x < 0) u = -1.0f - eps; else if (x >= res) u = 1.0f + eps;
    if (y < 0) v = -1.0f - eps; else if (y >= res) v = 1.0f + eps;
    const FaceUV f = dir_to_face(face_to_dir(face, u, v));
    int xi = (int)floorf((f.u * 0.5f + 0.5f) * (float)res);
    int yi = (int)floorf((f.v * 0.5f + 0.5f) * (float)res);
    xi = min(max(xi, 0), res - 1);
    yi = min(max(yi, 0), res - 1);
    return (f.face * res + yi) * res + xi;
}
__device__ __forceinline__ Taps cube_taps(const FaceUV& f, int res)
{
    Taps t;
    const float fx = (f.u * 0.5f + 0.5f) * (float)res - 0.5f;
    const float fy = (f.v * 0.5f + 0.5f) * (float)res - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    t.wx = fx - x0f; t.wy = fy - y0f;
    const bool ox0 = x0 < 0, ox1 = x0 + 1 >= res, oy0 = y0 < 0, oy1 = y0 + 1 >= res;
    t.w[0] = (1.f - t.wx) * (1.f - t.wy); t.w[1] = t.wx * (1.f - t.wy); t.w[2] = (1.f - t.wx) * t.wy; t.w[3] = t.wx * t.wy;
    const bool c0 = ox0 && oy0, c1 = ox1 && oy0, c2 = ox0 && oy1, c3 = ox1 && oy1;
    t.corner = c0 || c1 || c2 || c3;
    t.norm = 1.0f;
    if (t.corner) {   // three faces meet: the diagonal tap does not exist
        if (c0) t.w[0] = 0.f; if (c1) t.w[1] = 0.f; if (c2) t.w[2] = 0.f; if (c3) t.w[3] = 0.f;
        const float s = shade_rcp(t.w[0] + t.w[1] + t.w[2] + t.w[3]);
        t.norm = s;
        t.w[0] *= s; t.w[1] *= s; t.w[2] *= s; t.w[3] *= s;
    }
    t.idx[0] = c0 ? 0 : wrap_tap(f.face, x0, y0, res);
    t.idx[1] = c1 ? 0 : wrap_tap(f.face, x0 + 1, y0, res);
    t.idx[2] = c2 ? 0 : wrap_tap(f.face, x0, y0 + 1, res);
    t.idx[3] = c3 ? 0 : wrap_tap(f.face, x0 + 1, y0 + 1, res);
    return t;
}

// get_mip, scene/light.py:88-96 (n = number of specular levels); dlevel = d level / d roughness
__device__ __forceinline__ float mip_level(const EnvMips& m, float r, float& dlevel)
{
    const float lo = m.min_roughness, hi = m.max_roughness;
    const float n2 = (float)(m.n - 2);
    // (the two slopes are uniform: one scalar-sourced reciprocal each instead of a quotient per lane)
    const float inv_a = shade_rcp(hi - lo), inv_b = shade_rcp(1.0f - hi);
    if (r < hi) {
        const float c = fminf(fmaxf(r, lo), hi);
        dlevel = (r >= lo && r <= hi) ? n2 * inv_a : 0.f;
        return (c - lo) * inv_a * n2;
    }
    const float c = fminf(fmaxf(r, hi), 1.0f);
    dlevel = (r >= hi && r <= 1.0f) ? inv_b : 0.f;
    return (c - hi) * inv_b + n2;
}

struct __attribute__((aligned(4))) Tex3 { float x, y, z; };     // one texel: a 12-byte load at 4-byte alignment
struct EnvSample { float L[3]; float dlev[3]; float du[2][3], dv[2][3]; int l0, l1; float f; bool lev_in; };

// per-lane level -> its resolution / texels by a select chain over the (scalar) kernel arguments: indexing the by-value struct with a
// lane-dependent level is a memory round trip of its own in front of the texel loads
__device__ __forceinline__ int level_res(const EnvMips& m, int l)
{
    int r = m.res[0];
#pragma unroll
    for (int i = 1; i < MRGS_MAX_MIPS; i++) r = (l == i) ? m.res[i] : r;
    return r;
}
__device__ __forceinline__ const float* level_tex(const EnvMips& m, int l)
{
    const float* p = m.tex[0];
#pragma unroll
    for (int i = 1; i < MRGS_MAX_MIPS; i++) p = (l == i) ? m.tex[i] : p;
    return p;
}

// the two levels a fetch blends and the blend factor (s.l0, s.l1, s.f, s.lev_in)
__device__ __forceinline__ void env_levels(const EnvMips& m, float level, bool use_mips, EnvSample& s)
{
    const int top = use_mips ? m.n - 1 : 0;
    const float lc = fminf(fmaxf(level, 0.f), (float)top);
    s.lev_in = level >= 0.f && level <= (float)top;
    s.l0 = min((int)floorf(lc), top);
    s.l1 = min(s.l0 + 1, top);
    s.f = lc - (float)s.l0;
}

// trilinear seamless cube fetch (pre-sigmoid); fills what the backward needs
__device__ __forceinline__ void env_fetch(const EnvMips& m, const FaceUV& fu, float level, bool use_mips, EnvSample& s, Taps tp[2])
{
    env_levels(m, level, use_mips, s);
    float v[2][3];
    // the taps of both levels first, then all eight 12-byte texel loads in flight together (unconditional: a missing corner tap has
    // index 0 and weight 0 -- behind a condition every load waited for the one before)
    const int res0 = level_res(m, s.l0), res1 = level_res(m, s.l1);
    tp[0] = cube_taps(fu, res0);
    tp[1] = cube_taps(fu, res1);
    const float* tex0 = level_tex(m, s.l0);
    const float* tex1 = level_tex(m, s.l1);
    float t[2][4][3];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const Tex3 v3 = *reinterpret_cast<const Tex3*>((k == 0 ? tex0 : tex1) + (size_t)tp[k].idx[q] * 3);
            t[k][q][0] = v3.x; t[k][q][1] = v3.y; t[k][q][2] = v3.z;
        }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int res = k == 0 ? res0 : res1;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int c = 0; c < 3; c++) t[k][q][c] = tp[k].w[q] != 0.f ? t[k][q][c] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[k][c] = tp[k].w[0] * t[k][0][c] + tp[k].w[1] * t[k][1][c] + tp[k].w[2] * t[k][2][c] + tp[k].w[3] * t[k][3][c];
            // d value / d fx, d value / d fy (bilinear; the corner renormalisation is treated as constant)
            s.du[k][c] = ((1.f - tp[k].wy) * (t[k][1][c] - t[k][0][c]) + tp[k].wy * (t[k][3][c] - t[k][2][c])) * 0.5f * (float)res * tp[k].norm;
            s.dv[k][c] = ((1.f - tp[k].wx) * (t[k][2][c] - t[k][0][c]) + tp[k].wx * (t[k][3][c] - t[k][1][c])) * 0.5f * (float)res * tp[k].norm;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        s.L[c] = (1.f - s.f) * v[0][c] + s.f * v[1][c];
        s.dlev[c] = (s.lev_in && s.l1 != s.l0) ? v[1][c] - v[0][c] : 0.f;
    }
}

// v_rcp / v_exp form, a few ulp from the IEEE sigmoidf of mrgs_model_math.h (which the per-gaussian kernels use)
__device__ __forceinline__ float sigmoid_fast(float x) { return shade_rcp(1.0f + __expf(-x)); }

// Add v[0..2] to the texel at `addr` (nullptr / all-zero v = nothing to add).  Neighbouring pixels mirror into the same few
// texels (every lane of a wave into ONE texel of the coarse mip levels), and same-address atomics of one instruction
// serialise in L2: combine the lanes that share a texel inside the wave first (leader election by ballot, DPP sums), for at
// most MAX_ROUNDS distinct texels, and let the rest fall through to plain atomics.  Convergent: every lane of the wave calls it.
__device__ __forceinline__ void texel_scatter(float* addr, const float v[3])
{
    const int MAX_ROUNDS = 4;
    bool pending = addr != nullptr && (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f);
    const unsigned lo = (unsigned)(uintptr_t)addr, hi = (unsigned)((uintptr_t)addr >> 32);
    for (int r = 0; r < MAX_ROUNDS; r++) {
        const unsigned long long pm = __ballot(pending);
        if (pm == 0ull) return;
        const int leader = __builtin_ctzll(pm);
        const unsigned klo = __builtin_amdgcn_readlane(lo, leader), khi = __builtin_amdgcn_readlane(hi, leader);
        const bool match = pending && lo == klo && hi == khi;
        const float s0 = wave_dpp_sum(match ? v[0] : 0.f), s1 = wave_dpp_sum(match ? v[1] : 0.f), s2 = wave_dpp_sum(match ? v[2] : 0.f);
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(addr + 0, s0);
            atomicAdd(addr + 1, s1);
            atomicAdd(addr + 2, s2);
        }
        pending = pending && !match;
    }
    if (pending) {
        atomicAdd(addr + 0, v[0]);
        atomicAdd(addr + 1, v[1]);
        atomicAdd(addr + 2, v[2]);
    }
}

// gradient of the fetch: scatter to the texels (global atomics, lanes sharing a texel combined by texel_scatter; SCATTER = false leaves the
// texels to the caller), return d/d dir and d/d level
template <bool SCATTER = true>
__device__ __forceinline__ void env_fetch_bwd(const EnvMips& m, const FaceUV& fu, f3 dir, const EnvSample& s, const Taps tp[2],
                                              const float gL[3], f3& g_dir, float& g_level)
{
    float gu = 0.f, gv = 0.f;
    g_level = 0.f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const float wk = k == 0 ? 1.f - s.f : s.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float g = gL[c] * wk;
            gu += g * s.du[k][c];
            gv += g * s.dv[k][c];
        }
        if constexpr (SCATTER) {
            const int lk = k == 0 ? s.l0 : s.l1;
            float* gt = m.grad[lk];
            if (gt != nullptr) {   // privatised copy of this workgroup
                const unsigned wg = blockIdx.x + blockIdx.y * gridDim.x;
                gt += (size_t)(wg % (unsigned)m.copies[lk]) * (size_t)(6 * m.res[lk] * m.res[lk] * 3);
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float wq = wk * tp[k].w[q];
                const float vq[3] = {gL[0] * wq, gL[1] * wq, gL[2] * wq};
                texel_scatter((gt != nullptr && wq != 0.f) ? gt + (size_t)tp[k].idx[q] * 3 : nullptr, vq);     // wave-convergent
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) g_level += gL[c] * s.dlev[c];
    // (u, v) = (su * a, sv * b) / |major|  ->  d/d dir
    float ga = gu * fu.inv_ma, gb = gv * fu.inv_ma;                       // w.r.t. the signed minor components
    const float gm = -(gu * fu.u + gv * fu.v) * fu.sgn * fu.inv_ma;        // w.r.t. the major component
    g_dir = mk(0.f, 0.f, 0.f);
    switch (fu.face) {
    case 0: g_dir = mk(gm, -gb, -ga); break;   // u = -z/|x|, v = -y/|x|
    case 1: g_dir = mk(gm, -gb, ga); break;    // u = +z/|x|, v = -y/|x|
    case 2: g_dir = mk(ga, gm, gb); break;     // u = +x/|y|, v = +z/|y|
    case 3: g_dir = mk(ga, gm, -gb); break;    // u = +x/|y|, v = -z/|y|
    case 4: g_dir = mk(ga, -gb, gm); break;    // u = +x/|z|, v = -y/|z|
    default: g_dir = mk(-ga, -gb, gm); break;  // u = -x/|z|, v = -y/|z|
    }
    (void)dir;
}

// the split-sum FG LUT ([lres, lres, 2], `clamp` boundary): value and d/du, d/dv
__device__ __forceinline__ void lut_fetch(const float* __restrict__ lut, int lres, float u, float v, float fg[2], float du[2], float dv[2])
{
    const float fx = u * (float)lres - 0.5f, fy = v * (float)lres - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx = fx - x0f, wy = fy - y0f;
    const int x0 = min(max((int)x0f, 0), lres - 1), x1 = min(max((int)x0f + 1, 0), lres - 1);
    const int y0 = min(max((int)y0f, 0), lres - 1), y1 = min(max((int)y0f + 1, 0), lres - 1);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float t00 = lut[((size_t)y0 * lres + x0) * 2 + c], t10 = lut[((size_t)y0 * lres + x1) * 2 + c];
        const float t01 = lut[((size_t)y1 * lres + x0) * 2 + c], t11 = lut[((size_t)y1 * lres + x1) * 2 + c];
        fg[c] = (1.f - wy) * ((1.f - wx) * t00 + wx * t10) + wy * ((1.f - wx) * t01 + wx * t11);
        du[c] = ((1.f - wy) * (t10 - t00) + wy * (t11 - t01)) * (float)lres;
        dv[c] = ((1.f - wx) * (t01 - t00) + wx * (t11 - t10)) * (float)lres;
    }
}

// ---- host side: the C ABI's mip chain -> the kernel argument (every level checked; lds_off left at "global only") ----------------------
static inline int make_mips(const MrgsEnvMips* in, EnvMips& m)
{
    if (!in || in->n_levels < 1 || in->n_levels > MRGS_MAX_MIPS) return MRGS_E_BAD_ARG;
    m.n = in->n_levels;
    for (int i = 0; i < MRGS_MAX_MIPS; i++) {
        m.res[i] = i < m.n ? in->res[i] : 0;
        m.tex[i] = i < m.n ? in->tex[i] : nullptr;
        m.grad[i] = i < m.n ? in->grad[i] : nullptr;
        m.copies[i] = (i < m.n && in->grad_copies[i] > 1) ? in->grad_copies[i] : 1;
        m.lds_off[i] = -1;
        if (i < m.n && (!m.tex[i] || m.res[i] < 1)) return MRGS_E_BAD_ARG;
    }
    m.min_roughness = in->min_roughness;
    m.max_roughness = in->max_roughness;
    return MRGS_OK;
}
