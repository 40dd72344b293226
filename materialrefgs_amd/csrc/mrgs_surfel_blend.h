// mrgs_surfel_blend.h -- the surfel tracer's compositing arithmetic and the parts of its hand-written adjoint that exist once.
//
// mrgs_surfel_trace.hip is compiled with -ffp-contract=off on the promise that the forward, the backward that walks again, the backward that
// replays the record and the one-ray-per-wave path evaluate the same expressions on the same operands.  Stated here and called from both
// tracing functions: the hit (st_hit), a ray's upstream gradients and forward totals (StRayGrad), the contraction q of a hit (st_hit_q),
// the merge of two lanes that hold the same surfel (st_merge_pair), the atomics of a surfel's 18 terms and the per-ray writes.
// `Args` is the trace kernels' argument block (StArgs of mrgs_surfel_trace.hip).  Structs and sums travel BY VALUE, float by float:
// through references to the callers' loop-carried arrays the kernels compile to another instruction stream (tools/isa_digest.py).
#pragma once
#include "mrgs_surfel_trace.h"
#include "mrgs_wave.h"

namespace {

struct StHit { float t, u, v, G, alpha, den; bool ok; };

__device__ __forceinline__ StHit st_hit(const float4 g0, const float4 g1, const float4 g2, const float opacity,
                                        float ox, float oy, float oz, float dx, float dy, float dz)
{
    StHit h;
    const float mx = g0.x, my = g0.y, mz = g0.z, ax = g0.w, ay = g1.x, az = g1.y, bx = g1.z, by = g1.w, bz = g2.x, nx = g2.y, ny = g2.z, nz = g2.w;
    h.den = nx * dx + ny * dy + nz * dz;
    const float num = nx * (mx - ox) + ny * (my - oy) + nz * (mz - oz);
    h.t = num / h.den;
    const float px = (ox + h.t * dx) - mx, py = (oy + h.t * dy) - my, pz = (oz + h.t * dz) - mz;
    h.u = ax * px + ay * py + az * pz;
    h.v = bx * px + by * py + bz * pz;
    h.G = expf(-0.5f * (h.u * h.u + h.v * h.v));
    h.alpha = fminf(0.99f, opacity * h.G);
    h.ok = h.t > 0.0f && fabsf(h.u) <= ST_EXTENT && fabsf(h.v) <= ST_EXTENT && h.alpha >= 1.0f / 255.0f && h.t < 1e30f;   // false for NaN
    return h;
}

// ---- the backward's per-ray and per-hit arithmetic -----------------------------------------------------------------------------
// What a ray brings to the backward.  With the forward's totals at hand, d/d alpha_i = T_i q_i - (Q - Q_i) / (1 - alpha_i) - T_final (g.bg) /
// (1 - alpha_i): q_i = the upstream gradient contracted with hit i's contribution (st_hit_q), Q = Qtot its weighted sum over all hits,
// Q_i over the hits up to and including i.
struct StRayGrad {
    float gc0, gc1, gc2, gd, ga, gn0, gn1, gn2, gx0, gx1, gdist;       // upstream gradients of rgb, dpt, acc, norm, aux, dist
    float fA, fM1, fM2, fT;                                            // the forward's acc, sum w t (= dpt), sum w t^2, final transmittance
    float bgdot, Qtot;
};

// Fills a zeroed R (both tracing functions).  3 r is formed once and 2 r per use because that is what keeps st_trace_tile's
// instruction stream.
template <class Args>
__device__ __forceinline__ void st_load_ray_grad(const Args& A, int64_t r, StRayGrad& R)
{
    const int64_t r3 = 3 * r;
    // (an upstream gradient nobody supplied is a null pointer = zeros: no zero-filled maps on the way in)
    if (A.g_rgb) { R.gc0 = A.g_rgb[r3]; R.gc1 = A.g_rgb[r3 + 1]; R.gc2 = A.g_rgb[r3 + 2]; }
    if (A.g_dpt) R.gd = A.g_dpt[r];
    if (A.g_acc) R.ga = A.g_acc[r];
    if (A.g_dist) R.gdist = A.g_dist[r];
    if (A.g_norm) { R.gn0 = A.g_norm[r3]; R.gn1 = A.g_norm[r3 + 1]; R.gn2 = A.g_norm[r3 + 2]; }
    if (A.g_aux) { R.gx0 = A.g_aux[2 * r]; R.gx1 = A.g_aux[2 * r + 1]; }
    R.fA = A.acc[r]; R.fM1 = A.dpt[r]; R.fM2 = A.state[4 * r]; R.fT = A.state[4 * r + 1];
    R.bgdot = R.gc0 * A.bg[0] + R.gc1 * A.bg[1] + R.gc2 * A.bg[2];
    R.Qtot = R.gc0 * (A.rgb[r3] - R.fT * A.bg[0]) + R.gc1 * (A.rgb[r3 + 1] - R.fT * A.bg[1]) + R.gc2 * (A.rgb[r3 + 2] - R.fT * A.bg[2])
           + R.gd * R.fM1 + R.ga * R.fA + R.gn0 * A.norm[r3] + R.gn1 * A.norm[r3 + 1] + R.gn2 * A.norm[r3 + 2]
           + R.gx0 * A.aux[2 * r] + R.gx1 * A.aux[2 * r + 1] + R.gdist * 2.0f * (R.fA * R.fM2 - R.fM1 * R.fM1);
}

// q of a hit at ray parameter t with attributes a0, a1 and the normal (nfx, nfy, nfz) turned against the ray
__device__ __forceinline__ float st_hit_q(const StRayGrad R, const float4 a0, const float4 a1, float t, float nfx, float nfy, float nfz)
{
    return R.gc0 * a0.x + R.gc1 * a0.y + R.gc2 * a0.z + R.gd * t + R.ga + R.gn0 * nfx + R.gn1 * nfy + R.gn2 * nfz
         + R.gx0 * a0.w + R.gx1 * a1.x + R.gdist * (t * t * R.fA - 2.0f * t * R.fM1 + R.fM2);
}

// The gradient of one blended hit -- from q, dalpha, du, dv, dp, dt, dnum, dden to the 13 geometry terms, the 5 attribute terms and the
// ray's own d o / d d -- is NOT a function here: st_trace_tile and st_trace_lone_rays each keep it written out, and the two copies must
// stay equal expression by expression.  As one function (terms through references, or returned by value) st_trace_kernel<1>, <2> and
// st_trace_rest_kernel<1> came out with the same instructions in other registers at best, with other scratch sizes at worst.

// a surfel's 18 terms go out: float atomics on its rows of g_geom and g_attr
template <class Args>
__device__ __forceinline__ void st_add_surfel_grad(const Args& A, uint32_t id, const float* gv)
{
    float* gg = A.g_geom + (size_t)id * 16;
#pragma unroll
    for (int k = 0; k < 13; ++k) atomicAdd(gg + k, gv[k]);
    float* ga_ = A.g_attr + (size_t)id * 8;
#pragma unroll
    for (int k = 0; k < 5; ++k) atomicAdd(ga_ + k, gv[13 + k]);
}

// ---- what a ray writes ------------------------------------------------------------------------------------------------------------
// (`state` stays with the callers: its fourth word differs, and the profiled build overwrites it)
template <class Args>
__device__ __forceinline__ void st_write_ray(const Args& A, int64_t r, float C0, float C1, float C2, float T, float D, float Aw, float dist, float N0, float N1,
                                             float N2, float X0, float X1)
{
    A.rgb[3 * r] = C0 + T * A.bg[0]; A.rgb[3 * r + 1] = C1 + T * A.bg[1]; A.rgb[3 * r + 2] = C2 + T * A.bg[2];
    A.dpt[r] = D; A.acc[r] = Aw; A.dist[r] = dist;
    A.norm[3 * r] = N0; A.norm[3 * r + 1] = N1; A.norm[3 * r + 2] = N2;
    A.aux[2 * r] = X0; A.aux[2 * r + 1] = X1;
}
template <class Args>
__device__ __forceinline__ void st_write_ray_grad(const Args& A, int64_t r, float go0, float go1, float go2, float gdir0, float gdir1, float gdir2)
{
    A.g_ray_o[3 * r] = go0; A.g_ray_o[3 * r + 1] = go1; A.g_ray_o[3 * r + 2] = go2;
    A.g_ray_d[3 * r] = gdir0; A.g_ray_d[3 * r + 1] = gdir1; A.g_ray_d[3 * r + 2] = gdir2;
}

// One step of the backward's lane merge: lanes `tid` and `tid ^ BIT` (CTRL: the DPP control word of that exchange) that are both live and
// hold the same surfel add their 18 gradient terms; the lower lane of the pair carries the sum, the upper one is done.
template <int CTRL, int BIT>
__device__ __forceinline__ void st_merge_pair(float (&gv)[18], uint32_t id, bool& live, int tid)
{
    const uint32_t pid = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)id, CTRL, 0xf, 0xf, true);
    const bool plive = __builtin_amdgcn_update_dpp(0, (int)live, CTRL, 0xf, 0xf, true) != 0;
    const bool merge = live && plive && pid == id;
    const bool lower = (tid & BIT) == 0;
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const float pv = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, gv[k]), CTRL, 0xf, 0xf, true));
        const float sum = gv[k] + pv;                    // (v_add_f32_dpp: the move folds into the add)
        gv[k] = (merge && lower) ? sum : gv[k];
    }
    live = live && !(merge && !lower);
}

// a value every lane holds alike, handed back through v_readfirstlane so that the compiler keeps it in a scalar register (which it
// cannot know by itself)
__device__ __forceinline__ float st_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// (Hillis-Steele inside the 16-lane DPP row: row_shr:1/2/4/8 with the identity for lanes whose source falls outside the row -- the same
// products / sums in the same order as the __shfl_up form these replace, without its five ds_bpermute round trips)
__device__ __forceinline__ float scan16_mul_excl(float v, int lane)          // exclusive prefix product over lanes 0..15 (others: don't care)
{
    float inc = v;
    inc *= MRGS_DPP(1.0f, inc, 0x111, 0xf); inc *= MRGS_DPP(1.0f, inc, 0x112, 0xf); inc *= MRGS_DPP(1.0f, inc, 0x114, 0xf); inc *= MRGS_DPP(1.0f, inc, 0x118, 0xf);
    return MRGS_DPP(1.0f, inc, 0x111, 0xf);
}
__device__ __forceinline__ float scan16_add_excl(float v, int lane)
{
    float inc = v;
    inc += MRGS_DPP(0.0f, inc, 0x111, 0xf); inc += MRGS_DPP(0.0f, inc, 0x112, 0xf); inc += MRGS_DPP(0.0f, inc, 0x114, 0xf); inc += MRGS_DPP(0.0f, inc, 0x118, 0xf);
    return MRGS_DPP(0.0f, inc, 0x111, 0xf);
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

}   // namespace
