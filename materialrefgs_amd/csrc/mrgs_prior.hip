// Per-pixel prior terms the training scripts add to the loss of one view outside calculate_loss, fused.
//
// Replaces mono_normal_loss (train_refnerf.py:202-251, train_glossy.py:212, train_refreal.py:190), the mask-entropy term on rend_alpha
// (train_refnerf.py:1210-1217, train_glossy.py:1274-1276) and the four ref-score material terms (train_refreal.py:1238-1258): in torch two
// matmuls, four normalize calls, two boolean-index gathers with their host waits and some sixty elementwise / reduction launches, and
// the same again in backward; here
//   prior_terms_fwd        one pass over the pixels by flat index (all maps are planar and contiguous): four pixels per thread in 16-byte
//                          accesses, a bounded grid with a grid-stride loop, the N mod 4 tail pixels by the
//                          first threads of workgroup 0.  Each pixel adds to NSUM partial sums, reduced in the wave, then over the four
//                          waves in a fixed order into one row per workgroup;
//   prior_terms_finalize   one workgroup sums the rows in double in a fixed order and writes the terms and their denominators;
//   prior_terms_bwd        one elementwise launch with the same indexing: upstream gradients and denominators come from device memory.
// No atomics: both directions are run-to-run identical.  No host read.  Definitions (N = H W pixels p, F.normalize(x) = x / max(|x|, 1e-12)):
//   normal prior   v = Rt X[:,p], a = normalize(v), b = normalize(prior[p]); l1 = sum_p m_p sum_c |a_c - b_c| / sum_p m_p, cos = sum_p m_p
//                  (1 - a.b) / sum_p m_p (m = 1 without a mask).  Where |v| < 1e-12 (background pixels of rend_normal are exactly 0) the
//                  clamp is active: a = v / 1e-12 and the gradient is g / 1e-12 without the projection term (torch's clamp_min backward).
//   mask entropy   o = clamp(alpha, 1e-6f, (float)(1 - 1e-6)); L = -mean(m log o + (1 - m) log(1 - o)); the gradient passes where
//                  lo <= alpha <= hi.
//   ref score      a1 = mean_S |refl - 0.9|, a2 = mean_S |rough - 0.05|, b1 = mean_notS |refl - 0.05|, b2 = mean_notS |0.9 - rough|.
// Every division is IEEE: an all-zero mask or an empty set gives NaN, as the reference does.
#include "mrgs_internal.h"
#include "mrgs_wave.h"

namespace {

constexpr int NSUM = 11;          // l1 / cos of surf, l1 / cos of rend, sum m, entropy, a1, a2, b1, b2, |S|
constexpr int ROW = 12;           // floats per workgroup row (three 16-byte words)
constexpr int PX = 4;             // pixels per thread and step
constexpr int MAX_BLOCKS = 1024;  // four workgroups per CU
constexpr float NORM_EPS = 1e-12f;
constexpr float ALPHA_LO = 1e-6f;
constexpr float ALPHA_HI = (float)(1.0 - 1e-6);

struct PriorMaps {
    int64_t N;
    float Rt[9];                                  // v = Rt x, row-major
    const float *surf, *rend, *prior, *mask;      // [3,N], [3,N], [N,3], [N] or null
    const float *alpha, *amask;                   // [N], [N]
    const float *refl, *rough;                    // [N], [N]
    const uint8_t* score;                         // [N]
};

struct PriorUpstream {           // device scalars, null = 0; denominators: the forward's out_terms
    const float* g[13];
    const float* terms;
    float *g_surf, *g_rend, *g_alpha, *g_refl, *g_rough;
    int live_surf, live_rend, live_alpha, live_ref;
};

// Four consecutive floats from p + i (i a multiple of 4) in one 16-byte access.  Only dword alignment is asked of the address, which is all
// a global access of any width needs on CDNA: a plane whose base is not 16-byte aligned (N mod 4 != 0 shifts the second and third plane
// of a [3,N] map) takes the same path, its wave reading the same 1 KiB shifted by a few bytes.
__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t i, float (&v)[PX]) { __builtin_memcpy(v, p + i, sizeof(v)); }
__device__ __forceinline__ void store4(float* __restrict__ p, int64_t i, const float (&v)[PX]) { __builtin_memcpy(p + i, v, sizeof(v)); }

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

struct Unit { float x, y, z, len; };     // normalize(v) and |v|
__device__ __forceinline__ Unit unit(float x, float y, float z)
{
    const float len = sqrtf(x * x + y * y + z * z), d = fmaxf(len, NORM_EPS);
    return {x / d, y / d, z / d, len};
}
__device__ __forceinline__ Unit rotated_unit(const float (&Rt)[9], float x, float y, float z)
{
    return unit(Rt[0] * x + Rt[1] * y + Rt[2] * z, Rt[3] * x + Rt[4] * y + Rt[5] * z, Rt[6] * x + Rt[7] * y + Rt[8] * z);
}

// ---- the values of one pixel, loaded PX at a time or singly ---------------------------------------------------------------------------
struct Pixel {
    float s[3], r[3], n[3], m, alpha, am, refl, rough;
    bool in_s;
};

struct Loader {
    const PriorMaps& a;
    bool want_surf, want_rend, want_alpha, want_ref;
    // pixels i .. i + 3, i a multiple of 4 and i + 3 < N
    __device__ __forceinline__ void quad(int64_t i, Pixel (&px)[PX]) const
    {
        float t[PX];
        if (want_surf | want_rend) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (want_surf) {
                    load4(a.surf + c * a.N, i, t);
#pragma unroll
                    for (int k = 0; k < PX; ++k) px[k].s[c] = t[k];
                }
                if (want_rend) {
                    load4(a.rend + c * a.N, i, t);
#pragma unroll
                    for (int k = 0; k < PX; ++k) px[k].r[c] = t[k];
                }
            }
            float n[3 * PX];                      // the interleaved prior: twelve consecutive floats
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                load4(a.prior, 3 * i + 4 * w, t);
#pragma unroll
                for (int k = 0; k < PX; ++k) n[4 * w + k] = t[k];
            }
#pragma unroll
            for (int k = 0; k < PX; ++k) { px[k].n[0] = n[3 * k]; px[k].n[1] = n[3 * k + 1]; px[k].n[2] = n[3 * k + 2]; px[k].m = 1.f; }
            if (a.mask) {
                load4(a.mask, i, t);
#pragma unroll
                for (int k = 0; k < PX; ++k) px[k].m = t[k];
            }
        }
        if (want_alpha) {
            load4(a.alpha, i, t);
#pragma unroll
            for (int k = 0; k < PX; ++k) px[k].alpha = t[k];
            if (a.amask == a.mask && (want_surf | want_rend)) {         // the image mask serves both groups: read once
#pragma unroll
                for (int k = 0; k < PX; ++k) px[k].am = px[k].m;
            } else {
                load4(a.amask, i, t);
#pragma unroll
                for (int k = 0; k < PX; ++k) px[k].am = t[k];
            }
        }
        if (want_ref) {
            load4(a.refl, i, t);
#pragma unroll
            for (int k = 0; k < PX; ++k) px[k].refl = t[k];
            load4(a.rough, i, t);
#pragma unroll
            for (int k = 0; k < PX; ++k) px[k].rough = t[k];
            if (((uintptr_t)a.score & 3) == 0) {                        // (wave-uniform) a byte map is only promised byte alignment
                const uint32_t w = *reinterpret_cast<const uint32_t*>(a.score + i);
#pragma unroll
                for (int k = 0; k < PX; ++k) px[k].in_s = ((w >> (8 * k)) & 0xFFu) != 0;
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k) px[k].in_s = a.score[i + k] != 0;
            }
        }
    }
    __device__ __forceinline__ void one(int64_t i, Pixel& p) const
    {
        if (want_surf | want_rend) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (want_surf) p.s[c] = a.surf[c * a.N + i];
                if (want_rend) p.r[c] = a.rend[c * a.N + i];
                p.n[c] = a.prior[3 * i + c];
            }
            p.m = a.mask ? a.mask[i] : 1.f;
        }
        if (want_alpha) { p.alpha = a.alpha[i]; p.am = a.amask[i]; }
        if (want_ref) { p.refl = a.refl[i]; p.rough = a.rough[i]; p.in_s = a.score[i] != 0; }
    }
};

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void accumulate(const PriorMaps& a, const Pixel& p, float (&acc)[NSUM])
{
    if (a.surf) {
        const Unit b = unit(p.n[0], p.n[1], p.n[2]);
        const Unit s = rotated_unit(a.Rt, p.s[0], p.s[1], p.s[2]), r = rotated_unit(a.Rt, p.r[0], p.r[1], p.r[2]);
        acc[0] += p.m * (fabsf(s.x - b.x) + fabsf(s.y - b.y) + fabsf(s.z - b.z));
        acc[1] += p.m * (1.f - (s.x * b.x + s.y * b.y + s.z * b.z));
        acc[2] += p.m * (fabsf(r.x - b.x) + fabsf(r.y - b.y) + fabsf(r.z - b.z));
        acc[3] += p.m * (1.f - (r.x * b.x + r.y * b.y + r.z * b.z));
        acc[4] += p.m;
    }
    if (a.alpha) {
        const float o = fminf(fmaxf(p.alpha, ALPHA_LO), ALPHA_HI);
        acc[5] -= p.am * logf(o) + (1.f - p.am) * logf(1.f - o);
    }
    if (a.refl) {
        // selects, not branches: a branch that picks which sum to add to turns the sums into an indexed array in scratch
        const float dm = fabsf(p.refl - (p.in_s ? 0.9f : 0.05f)), dr = p.in_s ? fabsf(p.rough - 0.05f) : fabsf(0.9f - p.rough);
        acc[6] += p.in_s ? dm : 0.f; acc[7] += p.in_s ? dr : 0.f; acc[8] += p.in_s ? 0.f : dm; acc[9] += p.in_s ? 0.f : dr;
        acc[10] += p.in_s ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void prior_terms_fwd(PriorMaps a, float* __restrict__ partials)
{
    __shared__ float red[4][ROW];
    const int tid = threadIdx.x;
    const Loader ld = {a, a.surf != nullptr, a.surf != nullptr, a.alpha != nullptr, a.refl != nullptr};
    float acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.f;
    const int64_t quads = a.N / PX, step = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < quads; q += step) {
        Pixel px[PX];
        ld.quad(q * PX, px);
#pragma unroll
        for (int k = 0; k < PX; ++k) accumulate(a, px[k], acc);
    }
    if (blockIdx.x == 0 && quads * PX + tid < a.N) {          // the N mod 4 tail
        Pixel p;
        ld.one(quads * PX + tid, p);
        accumulate(a, p, acc);
    }
    block_row_sum_256(acc, red, partials + (size_t)blockIdx.x * ROW);
}

// out[0..3] l1 / cos of surf, l1 / cos of rend, [4] entropy, [5..8] a1 a2 b1 b2, [9] sum m, [10] |S|, [11] |not S|, [12] a1 + a2 + b1 +
// b2 / 2, [13..15] 0.  The terms of a group that is off are 0.
__global__ __launch_bounds__(256) void prior_terms_finalize(PriorMaps a, const float* __restrict__ partials, int nblocks, float* __restrict__ out)
{
    __shared__ double red[4][NSUM];
    const int tid = threadIdx.x;
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    for (int b = tid; b < nblocks; b += 256) {                 // one row per thread and pass; the order of the additions is fixed
        const float4* p = reinterpret_cast<const float4*>(partials + (size_t)b * ROW);
        const float4 r0 = p[0], r1 = p[1], r2 = p[2];
        acc[0] += r0.x; acc[1] += r0.y; acc[2] += r0.z; acc[3] += r0.w; acc[4] += r1.x; acc[5] += r1.y; acc[6] += r1.z; acc[7] += r1.w;
        acc[8] += r2.x; acc[9] += r2.y; acc[10] += r2.z;
    }
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        const double v = wave_shfl_sum(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double s[NSUM];
        for (int k = 0; k < NSUM; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        for (int k = 0; k < 16; ++k) out[k] = 0.f;
        const double N = (double)a.N;
        if (a.surf) {
            for (int k = 0; k < 4; ++k) out[k] = (float)(s[k] / s[4]);
            out[9] = (float)s[4];
        }
        if (a.alpha) out[4] = (float)(s[5] / N);
        if (a.refl) {
            const double n_s = s[10], n_not = N - s[10];
            const float a1 = (float)(s[6] / n_s), a2 = (float)(s[7] / n_s), b1 = (float)(s[8] / n_not), b2 = (float)(s[9] / n_not);
            out[5] = a1; out[6] = a2; out[7] = b1; out[8] = b2; out[10] = (float)n_s; out[11] = (float)n_not;
            out[12] = ((a1 + a2) + b1) + 0.5f * b2;
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
struct Scalars {
    float l1s, coss, l1r, cosr, inv_m;     // upstream of the four normal terms, 1 / sum m
    float ent;                             // -upstream / N
    float a1, a2, b1, b2;                  // upstream / |S|, / |not S| (the sum's upstream folded in)
};

// dL/dx of one map: x -> v = Rt x -> a = normalize(v); dL/da_c = k (g_l1 sign(a_c - b_c) - g_cos b_c)
__device__ __forceinline__ void normal_grad(const float (&Rt)[9], const float (&x)[3], const Unit& b, float k, float g_l1, float g_cos, float (&gx)[3])
{
    const Unit u = rotated_unit(Rt, x[0], x[1], x[2]);
    const float ga[3] = {k * (g_l1 * sgn(u.x - b.x) - g_cos * b.x), k * (g_l1 * sgn(u.y - b.y) - g_cos * b.y), k * (g_l1 * sgn(u.z - b.z) - g_cos * b.z)};
    float gv[3];
    if (u.len >= NORM_EPS) {
        const float dot = u.x * ga[0] + u.y * ga[1] + u.z * ga[2];
        gv[0] = (ga[0] - u.x * dot) / u.len; gv[1] = (ga[1] - u.y * dot) / u.len; gv[2] = (ga[2] - u.z * dot) / u.len;
    } else {                                // the clamp is active: no projection term
        gv[0] = ga[0] / NORM_EPS; gv[1] = ga[1] / NORM_EPS; gv[2] = ga[2] / NORM_EPS;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) gx[c] = Rt[c] * gv[0] + Rt[3 + c] * gv[1] + Rt[6 + c] * gv[2];      // the transpose of Rt: back to world space
}

struct PixelGrad { float s[3], r[3], alpha, refl, rough; };

__device__ __forceinline__ void pixel_grad(const PriorMaps& a, const PriorUpstream& u, const Scalars& sc, const Pixel& p, PixelGrad& g)
{
    if (u.live_surf | u.live_rend) {
        const Unit b = unit(p.n[0], p.n[1], p.n[2]);
        const float k = p.m * sc.inv_m;
        if (u.live_surf) normal_grad(a.Rt, p.s, b, k, sc.l1s, sc.coss, g.s);
        if (u.live_rend) normal_grad(a.Rt, p.r, b, k, sc.l1r, sc.cosr, g.r);
    }
    if (u.live_alpha) {
        const bool pass = (p.alpha >= ALPHA_LO) & (p.alpha <= ALPHA_HI);
        g.alpha = pass ? sc.ent * (p.am / p.alpha - (1.f - p.am) / (1.f - p.alpha)) : 0.f;
    }
    if (u.live_ref) {
        g.refl = p.in_s ? sc.a1 * sgn(p.refl - 0.9f) : sc.b1 * sgn(p.refl - 0.05f);
        g.rough = p.in_s ? sc.a2 * sgn(p.rough - 0.05f) : -sc.b2 * sgn(0.9f - p.rough);
    }
}

__global__ __launch_bounds__(256) void prior_terms_bwd(PriorMaps a, PriorUpstream u)
{
    const int tid = threadIdx.x;
    auto up = [&](int k) { return u.g[k] ? u.g[k][0] : 0.f; };
    Scalars sc = {};
    if (u.live_surf | u.live_rend) { sc.l1s = up(0); sc.coss = up(1); sc.l1r = up(2); sc.cosr = up(3); sc.inv_m = 1.f / u.terms[9]; }
    if (u.live_alpha) sc.ent = -up(4) / (float)a.N;
    if (u.live_ref) {
        const float sum = up(12), n_s = u.terms[10], n_not = u.terms[11];
        sc.a1 = (up(5) + sum) / n_s; sc.a2 = (up(6) + sum) / n_s; sc.b1 = (up(7) + sum) / n_not; sc.b2 = (up(8) + 0.5f * sum) / n_not;
    }
    const Loader ld = {a, u.live_surf != 0, u.live_rend != 0, u.live_alpha != 0, u.live_ref != 0};
    const int64_t quads = a.N / PX, step = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < quads; q += step) {
        const int64_t i = q * PX;
        Pixel px[PX];
        PixelGrad g[PX] = {};               // the maps of a group without an upstream gradient are written as zeros
        ld.quad(i, px);
#pragma unroll
        for (int k = 0; k < PX; ++k) pixel_grad(a, u, sc, px[k], g[k]);
        float t[PX];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (u.g_surf) {
#pragma unroll
                for (int k = 0; k < PX; ++k) t[k] = g[k].s[c];
                store4(u.g_surf + c * a.N, i, t);
            }
            if (u.g_rend) {
#pragma unroll
                for (int k = 0; k < PX; ++k) t[k] = g[k].r[c];
                store4(u.g_rend + c * a.N, i, t);
            }
        }
        if (u.g_alpha) {
#pragma unroll
            for (int k = 0; k < PX; ++k) t[k] = g[k].alpha;
            store4(u.g_alpha, i, t);
        }
        if (u.g_refl) {
#pragma unroll
            for (int k = 0; k < PX; ++k) t[k] = g[k].refl;
            store4(u.g_refl, i, t);
        }
        if (u.g_rough) {
#pragma unroll
            for (int k = 0; k < PX; ++k) t[k] = g[k].rough;
            store4(u.g_rough, i, t);
        }
    }
    if (blockIdx.x == 0 && quads * PX + tid < a.N) {
        const int64_t i = quads * PX + tid;
        Pixel p;
        PixelGrad g = {};
        ld.one(i, p);
        pixel_grad(a, u, sc, p, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (u.g_surf) u.g_surf[c * a.N + i] = g.s[c];
            if (u.g_rend) u.g_rend[c * a.N + i] = g.r[c];
        }
        if (u.g_alpha) u.g_alpha[i] = g.alpha;
        if (u.g_refl) u.g_refl[i] = g.refl;
        if (u.g_rough) u.g_rough[i] = g.rough;
    }
}

int prior_blocks(int64_t N)
{
    const int64_t b = (N / PX + 255) / 256;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

// the checks both directions share: the config, and that every group has all of its pointers or none
int make_maps(const MrgsPriorConfig* cfg, const float* Rt, const float* surf_normal, const float* rend_normal, const float* prior, const float* mask,
              const float* rend_alpha, const float* alpha_mask, const float* refl, const float* rough, const uint8_t* ref_score, PriorMaps& a)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsPriorConfig) || cfg->H <= 0 || cfg->W <= 0 || cfg->flags != 0) return MRGS_E_BAD_ARG;
    const int n_normal = (surf_normal != nullptr) + (rend_normal != nullptr) + (prior != nullptr);
    const int n_alpha = (rend_alpha != nullptr) + (alpha_mask != nullptr);
    const int n_ref = (refl != nullptr) + (rough != nullptr) + (ref_score != nullptr);
    if ((n_normal != 0 && n_normal != 3) || (n_alpha != 0 && n_alpha != 2) || (n_ref != 0 && n_ref != 3)) return MRGS_E_BAD_ARG;
    if (n_normal + n_alpha + n_ref == 0) return MRGS_E_BAD_ARG;
    if (n_normal ? !Rt : mask != nullptr) return MRGS_E_BAD_ARG;
    a.N = (int64_t)cfg->H * cfg->W;
    for (int k = 0; k < 9; ++k) a.Rt[k] = n_normal ? Rt[k] : 0.f;
    a.surf = surf_normal; a.rend = rend_normal; a.prior = prior; a.mask = mask;
    a.alpha = rend_alpha; a.amask = alpha_mask; a.refl = refl; a.rough = rough; a.score = ref_score;
    return MRGS_OK;
}

}   // namespace

extern "C" size_t mrgs_prior_ws_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return 0;
    return (size_t)prior_blocks((int64_t)H * W) * ROW * sizeof(float);
}

extern "C" int mrgs_prior_terms_forward(const MrgsPriorConfig* cfg, const float* Rt, const float* surf_normal, const float* rend_normal,
                                        const float* prior, const float* mask, const float* rend_alpha, const float* alpha_mask, const float* refl,
                                        const float* rough, const uint8_t* ref_score, void* ws, size_t ws_bytes, float* out_terms, void* stream)
{
    PriorMaps a;
    if (int rc = make_maps(cfg, Rt, surf_normal, rend_normal, prior, mask, rend_alpha, alpha_mask, refl, rough, ref_score, a)) return rc;
    if (!ws || !out_terms || ((uintptr_t)ws & 15) || ws_bytes < mrgs_prior_ws_bytes(cfg->H, cfg->W)) return MRGS_E_BAD_ARG;
    const int nblocks = prior_blocks(a.N);
    hipStream_t st = (hipStream_t)stream;
    prior_terms_fwd<<<nblocks, 256, 0, st>>>(a, (float*)ws);
    prior_terms_finalize<<<1, 256, 0, st>>>(a, (const float*)ws, nblocks, out_terms);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_prior_terms_backward(const MrgsPriorConfig* cfg, const float* Rt, const float* surf_normal, const float* rend_normal,
                                         const float* prior, const float* mask, const float* rend_alpha, const float* alpha_mask, const float* refl,
                                         const float* rough, const uint8_t* ref_score, const float* fwd_terms, const float* const* g_terms,
                                         float* g_surf_normal, float* g_rend_normal, float* g_alpha, float* g_refl, float* g_rough, void* stream)
{
    PriorMaps a;
    if (int rc = make_maps(cfg, Rt, surf_normal, rend_normal, prior, mask, rend_alpha, alpha_mask, refl, rough, ref_score, a)) return rc;
    if (!fwd_terms || !g_terms) return MRGS_E_BAD_ARG;
    if ((!a.surf && (g_surf_normal || g_rend_normal)) || (!a.alpha && g_alpha) || (!a.refl && (g_refl || g_rough))) return MRGS_E_BAD_ARG;
    if (!g_surf_normal && !g_rend_normal && !g_alpha && !g_refl && !g_rough) return MRGS_OK;        // nothing to write
    PriorUpstream u;
    for (int k = 0; k < 13; ++k) u.g[k] = g_terms[k];
    u.terms = fwd_terms;
    u.g_surf = g_surf_normal; u.g_rend = g_rend_normal; u.g_alpha = g_alpha; u.g_refl = g_refl; u.g_rough = g_rough;
    // a group whose upstream gradients are all NULL costs no loads and no arithmetic: its maps are written as zeros
    u.live_surf = g_surf_normal && (u.g[0] || u.g[1]);
    u.live_rend = g_rend_normal && (u.g[2] || u.g[3]);
    u.live_alpha = g_alpha && u.g[4];
    u.live_ref = (g_refl || g_rough) && (u.g[5] || u.g[6] || u.g[7] || u.g[8] || u.g[12]);
    prior_terms_bwd<<<prior_blocks(a.N), 256, 0, (hipStream_t)stream>>>(a, u);
    return MRGS_LAUNCH_STATUS();
}
