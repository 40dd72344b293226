// mrgs_bounce.hip -- one-bounce light from the material mesh on gfx950: bounce_shade_{fwd,bwd}_kernel and their two entry points.
//
// RayTracer.secondary_indirect_color (raytracing_brdf/raytracer.py:218-271) over the outputs of mrgs_bvh_trace, one ray per lane: a miss
// reads the un-filtered base level along -v, a hit gathers the three vertices of its triangle (3 x 12 B positions, 3 x 48 B attribute rows,
// uncoalesced: served by L2 / the Infinity Cache), interpolates with the reference's xy-projected area weights and shades with the split-sum
// terms against the prefiltered chain.  The fetch, its adjoint and the FG LUT fetch are those of mrgs_envmap.h.  The contract is in
// include/mrgs.h.
#include "mrgs_envmap.h"

struct BounceArgs {
    long long N, V, T;
    const float *pos, *view, *depth;
    const int* ids;
    const unsigned char* active;
    const float* vertices;
    const int* triangles;
    const float* table;      // [V,12]: diffuse 3, albedo 3, metallic, roughness | normal 3, pad
    const float* lut;
    int lres;
};

struct BounceHit {
    int iv[3];
    float w[3];              // area weights (not normalised to one)
    float diffuse[3], albedo[3], metallic, rough;
    f3 n, l;
    float ndv;
};

// the gather and the interpolation of one hit ray; false = the ray writes 0 (no such triangle, or a projected area of exactly 0)
__device__ __forceinline__ bool bounce_gather(const BounceArgs& a, long long i, BounceHit& h)
{
    const int id = a.ids[i];
    if (id < 0 || (long long)id >= a.T) return false;
    const int* tri = a.triangles + (size_t)id * 3;
    h.iv[0] = tri[0]; h.iv[1] = tri[1]; h.iv[2] = tri[2];
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (h.iv[k] < 0 || (long long)h.iv[k] >= a.V) return false;
    float vx[3], vy[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        vx[k] = a.vertices[(size_t)h.iv[k] * 3];
        vy[k] = a.vertices[(size_t)h.iv[k] * 3 + 1];
    }
    // barycentric_interpolation (:209-216): areas of the xy-projection, from differences to vertex a
    const float px = a.pos[3 * i] - vx[0], py = a.pos[3 * i + 1] - vy[0];
    const float bx = vx[1] - vx[0], by = vy[1] - vy[0], cx = vx[2] - vx[0], cy = vy[2] - vy[0];
    const float den = fabsf(bx * cy - cx * by);
    if (!(den > 0.f)) return false;                                   // (also a NaN area)
    h.w[0] = fabsf((bx - px) * (cy - py) - (cx - px) * (by - py)) / den;
    h.w[1] = fabsf(cx * py - cy * px) / den;
    h.w[2] = fabsf(px * by - py * bx) / den;
    float r[12];
#pragma unroll
    for (int c = 0; c < 12; c++) r[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4* row = reinterpret_cast<const float4*>(a.table + (size_t)h.iv[k] * 12);
        const float4 q0 = row[0], q1 = row[1], q2 = row[2];
        const float q[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int c = 0; c < 11; c++) r[c] = fmaf(h.w[k], q[c], r[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { h.diffuse[c] = r[c]; h.albedo[c] = r[3 + c]; }
    h.metallic = r[6]; h.rough = r[7];
    h.n = mk(r[8], r[9], r[10]);
    const f3 v = mk(a.view[3 * i], a.view[3 * i + 1], a.view[3 * i + 2]);
    h.ndv = dot3(h.n, v);                                             // reflection (utils/refl_utils.py:95-98), n as interpolated
    const f3 l = mk(2.f * h.n.x * h.ndv - v.x, 2.f * h.n.y * h.ndv - v.y, 2.f * h.n.z * h.ndv - v.z);
    const float inv = 1.0f / fmaxf(sqrtf(dot3(l, l)), 1e-20f);        // safe_normalize
    h.l = mk(l.x * inv, l.y * inv, l.z * inv);
    return true;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

__global__ void __launch_bounds__(256) bounce_shade_fwd_kernel(EnvMips m, EnvMips mb, BounceArgs a, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N) return;
    float o[3] = {0.f, 0.f, 0.f};
    if (a.active == nullptr || a.active[i] != 0) {
        EnvSample s;
        Taps tp[2];
        if (a.depth[i] >= 10.f) {                                     // left the scene: the environment itself
            env_fetch(mb, dir_to_face(mk(-a.view[3 * i], -a.view[3 * i + 1], -a.view[3 * i + 2])), 0.f, false, s, tp);
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = sigmoid_fast(s.L[c]);
        } else {
            BounceHit h;
            if (bounce_gather(a, i, h)) {
                float fg[2], du[2], dv[2], dl;
                lut_fetch(a.lut, a.lres, clamp01(h.ndv), clamp01(h.rough), fg, du, dv);
                env_fetch(m, dir_to_face(h.l), mip_level(m, h.rough, dl), true, s, tp);
                const float om = 1.f - h.metallic;
#pragma unroll
                for (int c = 0; c < 3; c++)
                    o[c] = om * h.diffuse[c] + ((0.04f * om + h.albedo[c] * h.metallic) * fg[0] + fg[1]) * sigmoid_fast(s.L[c]);
            }
        }
    }
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

// a fetch record whose backward adds nothing (weights 0, texel 0 of level 0)
__device__ __forceinline__ void bounce_null_fetch(EnvSample& s, Taps tp[2])
{
#pragma unroll
    for (int c = 0; c < 3; c++) { s.L[c] = 0.f; s.dlev[c] = 0.f; s.du[0][c] = s.du[1][c] = 0.f; s.dv[0][c] = s.dv[1][c] = 0.f; }
    s.l0 = s.l1 = 0; s.f = 0.f; s.lev_in = false;
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
        for (int q = 0; q < 4; q++) { tp[k].idx[q] = 0; tp[k].w[q] = 0.f; }
        tp[k].wx = tp[k].wy = 0.f; tp[k].norm = 1.f; tp[k].corner = false;
    }
}

// Recomputes the forward of its ray; the two texel scatters (base level for the misses, the chain for the hits) are wave-convergent, so
// every lane of the wave reaches both, with a null record where the fetch is not its own.
__global__ void __launch_bounds__(256) bounce_shade_bwd_kernel(EnvMips m, EnvMips mb, BounceArgs a, const float* __restrict__ g_out,
                                                               float* __restrict__ g_table)
{
    const long long i_ = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i_ < a.N;
    const long long i = valid ? i_ : a.N - 1;
    const bool live = valid && (a.active == nullptr || a.active[i] != 0);
    const float g[3] = {live ? g_out[3 * i] : 0.f, live ? g_out[3 * i + 1] : 0.f, live ? g_out[3 * i + 2] : 0.f};
    const bool miss = live && a.depth[i] >= 10.f;
    BounceHit h;
    const bool hit = live && !miss && bounce_gather(a, i, h);

    EnvSample s;
    Taps tp[2];
    FaceUV fu = dir_to_face(mk(1.f, 0.f, 0.f));
    float gL[3] = {0.f, 0.f, 0.f}, glev;
    f3 gd;
    bounce_null_fetch(s, tp);
    if (miss) {
        fu = dir_to_face(mk(-a.view[3 * i], -a.view[3 * i + 1], -a.view[3 * i + 2]));
        env_fetch(mb, fu, 0.f, false, s, tp);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float y = sigmoid_fast(s.L[c]);
            gL[c] = g[c] * y * (1.f - y);
        }
    }
    env_fetch_bwd<true>(mb, fu, mk(0.f, 0.f, 0.f), s, tp, gL, gd, glev);

    float fg[2] = {0.f, 0.f}, du[2], dv[2] = {0.f, 0.f}, dl = 0.f, light[3] = {0.f, 0.f, 0.f};
    gL[0] = gL[1] = gL[2] = 0.f;
    bounce_null_fetch(s, tp);
    if (hit) {
        lut_fetch(a.lut, a.lres, clamp01(h.ndv), clamp01(h.rough), fg, du, dv);
        fu = dir_to_face(h.l);
        env_fetch(m, fu, mip_level(m, h.rough, dl), true, s, tp);
        const float om = 1.f - h.metallic;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            light[c] = sigmoid_fast(s.L[c]);
            gL[c] = g[c] * ((0.04f * om + h.albedo[c] * h.metallic) * fg[0] + fg[1]) * light[c] * (1.f - light[c]);
        }
    }
    env_fetch_bwd<true>(m, fu, mk(0.f, 0.f, 0.f), s, tp, gL, gd, glev);

    if (!hit || g_table == nullptr) return;
    const float om = 1.f - h.metallic;
    float gr[8], g_fg0 = 0.f, g_fg1 = 0.f;
    gr[6] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float gw = g[c] * light[c];                             // d / d specular_weight
        gr[c] = g[c] * om;
        gr[3 + c] = gw * h.metallic * fg[0];
        gr[6] += -g[c] * h.diffuse[c] + gw * (h.albedo[c] - 0.04f) * fg[0];
        g_fg0 += gw * (0.04f * om + h.albedo[c] * h.metallic);
        g_fg1 += gw;
    }
    const bool v_in = h.rough >= 0.f && h.rough <= 1.f;               // the clamp of the table's v coordinate passes gradient on [0, 1]
    gr[7] = glev * dl + (v_in ? g_fg0 * dv[0] + g_fg1 * dv[1] : 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float* row = g_table + (size_t)h.iv[k] * 8;
#pragma unroll
        for (int c = 0; c < 8; c++) atomicAdd(row + c, h.w[k] * gr[c]);
    }
}

// ---- entry points --------------------------------------------------------------------------------------------
// the checks the two bounce entry points share; MRGS_OK with a.N == 0 = nothing to launch
static int bounce_args(const MrgsBounceConfig* cfg, const MrgsEnvMips* mips, const float* base, float* g_base, const float* hit_pos,
                       const float* rays_v, const int32_t* face_ids, const float* depth, const uint8_t* active, const float* vertices,
                       const int32_t* triangles, const float* table, const float* lut, EnvMips& m, EnvMips& mb, BounceArgs& a)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsBounceConfig) || cfg->flags != 0) return MRGS_E_BAD_ARG;
    if (cfg->n_rays < 0 || cfg->n_vertices < 0 || cfg->n_triangles < 0 || cfg->base_res < 1 || cfg->lut_res < 1) return MRGS_E_BAD_ARG;
    a.N = cfg->n_rays;
    if (a.N == 0) return MRGS_OK;
    if (int rc = make_mips(mips, m)) return rc;
    if (!base || !hit_pos || !rays_v || !face_ids || !depth || !vertices || !triangles || !table || !lut) return MRGS_E_BAD_ARG;
    if (((uintptr_t)table & 15) || cfg->n_vertices == 0 || cfg->n_triangles == 0) return MRGS_E_BAD_ARG;
    if (a.N >= (1ll << 31) * 256) return MRGS_E_UNSUPPORTED;
    mb = m;                                                           // the un-filtered base level as a chain of one
    mb.n = 1;
    for (int i = 0; i < MRGS_MAX_MIPS; i++) { mb.res[i] = 0; mb.tex[i] = nullptr; mb.grad[i] = nullptr; mb.copies[i] = 1; }
    mb.res[0] = cfg->base_res; mb.tex[0] = base; mb.grad[0] = g_base;
    a.V = cfg->n_vertices; a.T = cfg->n_triangles;
    a.pos = hit_pos; a.view = rays_v; a.depth = depth; a.ids = face_ids; a.active = active;
    a.vertices = vertices; a.triangles = triangles; a.table = table; a.lut = lut; a.lres = cfg->lut_res;
    return MRGS_OK;
}

extern "C" {

int mrgs_bounce_shade_forward(const MrgsBounceConfig* cfg, const MrgsEnvMips* mips, const float* base, const float* hit_pos, const float* rays_v,
                              const int32_t* face_ids, const float* depth, const uint8_t* active, const float* vertices, const int32_t* triangles,
                              const float* table, const float* lut, float* out, void* stream)
{
    EnvMips m, mb;
    BounceArgs a;
    if (int rc = bounce_args(cfg, mips, base, nullptr, hit_pos, rays_v, face_ids, depth, active, vertices, triangles, table, lut, m, mb, a)) return rc;
    if (a.N == 0) return MRGS_OK;
    if (!out) return MRGS_E_BAD_ARG;
    for (int i = 0; i < MRGS_MAX_MIPS; i++) m.grad[i] = nullptr;
    hipLaunchKernelGGL(bounce_shade_fwd_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, mb, a, out);
    return MRGS_LAUNCH_STATUS();
}

int mrgs_bounce_shade_backward(const MrgsBounceConfig* cfg, const MrgsEnvMips* mips, const float* base, float* g_base, const float* hit_pos,
                               const float* rays_v, const int32_t* face_ids, const float* depth, const uint8_t* active, const float* vertices,
                               const int32_t* triangles, const float* table, const float* lut, const float* g_out, float* g_table, void* stream)
{
    EnvMips m, mb;
    BounceArgs a;
    if (int rc = bounce_args(cfg, mips, base, g_base, hit_pos, rays_v, face_ids, depth, active, vertices, triangles, table, lut, m, mb, a)) return rc;
    if (a.N == 0) return MRGS_OK;
    if (!g_out) return MRGS_E_BAD_ARG;
    hipLaunchKernelGGL(bounce_shade_bwd_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, mb, a, g_out, g_table);
    return MRGS_LAUNCH_STATUS();
}

}   // extern "C"
