// Multi-view material consistency loss (calc_warp_loss, train_refnerf.py:414-739, train_glossy.py:442-772, train_refreal.py:405-729).
//
// Forward, all on the caller's stream and without a host read:
//   warp_geo_fwd        per pixel of view v: back-project through D_v, project into the neighbour n, read D_n there (bilinear, border,
//                       align_corners), back-project, re-project into v; e = |p' - p|, valid = in frustum and e < th, w = exp(-e) on valid
//                       pixels.  Double precision (the reprojection error is a small difference of ~10^3-pixel coordinates).  Writes the
//                       weight map, a valid byte map and one (sum w e, count) partial per workgroup.
//   warp_geo_finalize   one workgroup: the partials in a fixed order -> n_valid and the geometric term.
//   warp_sel_hist / warp_sel_scan (twice)   radix select of the k smallest per-pixel keys over the valid pixels.  The key is a seeded
//                       bijection of the pixel index, so keys never tie and the k smallest are one well-defined set.  warp_sel_scan: 64 bins a
//                       thread, block_exclusive_scan (mrgs_wave.h) over the 1024 sums, then one thread walks its bins.
//   warp_compact_count / warp_compact_scan / warp_compact_write   the selected pixels in ascending pixel order and the sample-slot map; the scan is
//                       block_counts_exclusive_scan (mrgs_wave.h), in place.
//   warp_patch_fwd      one 64-lane wave per sample, one lane per tap of the (2h+1)^2 patch: the view's taps at integer texels, the
//                       neighbour's through the sample's plane homography (bilinear, zeros, align_corners), wave reductions in a fixed
//                       order -> the per-sample base-colour, metallic and roughness terms.
//   warp_patch_finalize one workgroup: the per-sample terms in a fixed order -> the three material scalars.
// Backward:
//   warp_geo_bwd        per valid pixel: de/dD_v (through the neighbour lookup position as well) and the four border-mode corners of D_n
//                       (atomics).
//   warp_view_gather    per view pixel: the <= (2h+1)^2 samples whose patch covers it, found through the slot map; no atomics.
//   warp_nbr_scatter    per sample wave: the bilinear corners of every neighbour tap (atomics).
// Grey-image NCC (train_refreal.py's get_consistency_loss2), a second pair of calls on the same draw: warp_ncc_fwd / warp_ncc_finalize /
// warp_ncc_bwd, described where they stand at the end of the file.
// Reflection score (calc_ref_score, the producer of the ref-score loss's input): ref_score_fwd at the end of the file, one dense gather
// pass per view over all of its neighbours with the geometry, homography and bilinear helpers of the kernels above.
// The file is compiled with -ffp-contract=off: the tap positions of the backward kernels repeat the forward's arithmetic bit for bit.
#include "mrgs_internal.h"
#include "mrgs_wave.h"

namespace {

constexpr int WB = 256;                  // threads per workgroup of the per-pixel kernels
constexpr int FIN = 1024;                // threads of the single-workgroup reductions
constexpr int NBINS = 65536;             // radix-select bins per pass (16 bits)

// ws state words (int32)
constexpr int ST_NVALID = 0, ST_NSEL = 1, ST_TAKEALL = 2, ST_BIN = 3, ST_REM = 4, ST_THRESH = 5, ST_NKEEP = 6;
constexpr int ST_WORDS = 64;

struct WarpArgs {
    int H, W, k, h, P;                   // P = (2h+1)^2 taps
    int n_given;                         // >= 0: samples given by the caller
    uint32_t flags;
    uint32_t s0, s1;                     // key seeds
    double fxv, fyv, cxv, cyv, fxn, fyn, cxn, cyn;
    float th, geo_w, base_w, metal_w, rough_w;
};

struct WarpWs {
    int32_t* st;
    uint32_t* hist;                      // [2][NBINS]
    double* geo_part;                    // [nbg] sum of w e
    int32_t* cnt_part;                   // [nbg] valid pixels
    int32_t* blk;                        // [nbg] selected pixels per workgroup, then their exclusive scan
    uint8_t* valid;                      // [HW]
    int32_t* slot;                       // [HW] sample index or -1
    int32_t* samples;                    // [k] pixel indices
    double* homog;                       // [k][9]
    float4* rec;                         // [k] (w, L'(t_m) vw or 0, L'(t_r) or 0, keep)
    float* terms;                        // [3][k] base, L(t_m) (0 off keep), L(t_r) (0 off keep)
};

inline size_t al(size_t v) { return mrgs_align_up(v, 256); }

size_t ws_layout(int H, int W, int k, WarpWs* w, char* base)
{
    const size_t HW = (size_t)H * W, nbg = (HW + WB - 1) / WB;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return base ? base + at : nullptr; };
    char* st = take(ST_WORDS * 4);
    char* hist = take(2 * (size_t)NBINS * 4);
    char* gp = take(nbg * 8);
    char* cp = take(nbg * 4);
    char* bk = take(nbg * 4);
    char* va = take(HW);
    char* sl = take(HW * 4);
    char* sa = take((size_t)k * 4);
    char* ho = take((size_t)k * 9 * 8);
    char* re = take((size_t)k * 16);
    char* te = take((size_t)k * 3 * 4);
    if (w) {
        w->st = (int32_t*)st; w->hist = (uint32_t*)hist; w->geo_part = (double*)gp; w->cnt_part = (int32_t*)cp; w->blk = (int32_t*)bk;
        w->valid = (uint8_t*)va; w->slot = (int32_t*)sl; w->samples = (int32_t*)sa; w->homog = (double*)ho; w->rec = (float4*)re;
        w->terms = (float*)te;
    }
    return o;
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// a bijection of the pixel index (every step is invertible): distinct pixels never share a key
__device__ __forceinline__ uint32_t pixel_key(uint32_t idx, uint32_t s0, uint32_t s1)
{
    return fmix32(fmix32(fmix32(idx ^ s0) + s1) ^ s0);
}

// ---- geometry --------------------------------------------------------------------------------------------------------------------
// value and two derivatives: a = d/dD_v (total, the neighbour lookup position moves with D_v), b = d/dz_n (lookup value only)
struct D3 {
    double v, a, b;
};
__device__ __forceinline__ D3 mk(double v, double a = 0.0, double b = 0.0) { return D3{v, a, b}; }
__device__ __forceinline__ D3 operator+(D3 x, D3 y) { return D3{x.v + y.v, x.a + y.a, x.b + y.b}; }
__device__ __forceinline__ D3 operator-(D3 x, D3 y) { return D3{x.v - y.v, x.a - y.a, x.b - y.b}; }
__device__ __forceinline__ D3 operator*(D3 x, D3 y) { return D3{x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b}; }
__device__ __forceinline__ D3 operator*(D3 x, double c) { return D3{x.v * c, x.a * c, x.b * c}; }
__device__ __forceinline__ D3 operator/(D3 x, D3 y)
{
    const double q = x.v / y.v;
    return D3{q, (x.a - q * y.a) / y.v, (x.b - q * y.b) / y.v};
}

struct Cam {
    double Wm[4][4], R[3][3], T[3];
};

__device__ __forceinline__ void load_cam(const float* __restrict__ c, Cam& m)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) m.Wm[i][j] = (double)c[i * 4 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m.R[i][j] = (double)c[16 + i * 3 + j];
    for (int i = 0; i < 3; ++i) m.T[i] = (double)c[25 + i];
}

struct GeoOut {
    bool in_n;
    double e;
    D3 ex, ey;                           // p' - p with derivatives (valid only when in_n)
    int x0, y0;                          // border-clamped lookup corner
    double fx, fy;
};

// steps 1-5 of the statement for pixel (x, y), with the two derivatives of p' - p (camera records: world_view_transform 16, R 9, T 3)
__device__ __forceinline__ GeoOut geo_pixel(const WarpArgs& a, const Cam& cv, const Cam& cn, const float* __restrict__ Dn, int x, int y,
                                            float dv_f)
{
    GeoOut o;
    const D3 dv = mk((double)dv_f, 1.0, 0.0);
    const double rx = ((double)x - a.cxv) / a.fxv, ry = ((double)y - a.cyv) / a.fyv;
    D3 av[3] = {dv * rx - mk(cv.T[0]), dv * ry - mk(cv.T[1]), dv - mk(cv.T[2])};
    D3 X[3], q[3];
    for (int j = 0; j < 3; ++j) X[j] = av[0] * cv.R[j][0] + av[1] * cv.R[j][1] + av[2] * cv.R[j][2];
    for (int j = 0; j < 3; ++j) q[j] = X[0] * cn.Wm[0][j] + X[1] * cn.Wm[1][j] + X[2] * cn.Wm[2][j] + mk(cn.Wm[3][j]);
    const D3 ux = q[0] * a.fxn / q[2] + mk(a.cxn), uy = q[1] * a.fyn / q[2] + mk(a.cyn);
    o.in_n = ux.v > 0.0 && ux.v < (double)a.W && uy.v > 0.0 && uy.v < (double)a.H && q[2].v > 0.1;
    o.e = 0.0; o.ex = o.ey = mk(0.0); o.x0 = o.y0 = 0; o.fx = o.fy = 0.0;
    if (!o.in_n) return o;
    // border padding, align_corners: the position is clamped to [0, size-1] (zero gradient where it was clamped)
    const bool cx = ux.v > (double)(a.W - 1), cy = uy.v > (double)(a.H - 1);
    const double ix = cx ? (double)(a.W - 1) : ux.v, iy = cy ? (double)(a.H - 1) : uy.v;
    const int x0 = (int)floor(ix), y0 = (int)floor(iy);
    const double fx = ix - x0, fy = iy - y0;
    auto at = [&](int xx, int yy) -> double { return (xx < a.W && yy < a.H) ? (double)Dn[(size_t)yy * a.W + xx] : 0.0; };
    const double v00 = at(x0, y0), v01 = at(x0 + 1, y0), v10 = at(x0, y0 + 1), v11 = at(x0 + 1, y0 + 1);
    const double z = v00 * (1.0 - fx) * (1.0 - fy) + v01 * fx * (1.0 - fy) + v10 * (1.0 - fx) * fy + v11 * fx * fy;
    const double dzdx = cx ? 0.0 : ((v01 - v00) * (1.0 - fy) + (v11 - v10) * fy);
    const double dzdy = cy ? 0.0 : ((v10 - v00) * (1.0 - fx) + (v11 - v01) * fx);
    const D3 zn = mk(z, dzdx * ux.a + dzdy * uy.a, 1.0);
    D3 qp[3], Xp[3], pv[3];
    for (int j = 0; j < 3; ++j) qp[j] = q[j] / q[2] * zn;
    for (int j = 0; j < 3; ++j)
        Xp[j] = (qp[0] - mk(cn.T[0])) * cn.R[j][0] + (qp[1] - mk(cn.T[1])) * cn.R[j][1] + (qp[2] - mk(cn.T[2])) * cn.R[j][2];
    for (int j = 0; j < 3; ++j) pv[j] = Xp[0] * cv.Wm[0][j] + Xp[1] * cv.Wm[1][j] + Xp[2] * cv.Wm[2][j] + mk(cv.Wm[3][j]);
    o.ex = pv[0] * a.fxv / pv[2] + mk(a.cxv - (double)x);
    o.ey = pv[1] * a.fyv / pv[2] + mk(a.cyv - (double)y);
    o.e = sqrt(o.ex.v * o.ex.v + o.ey.v * o.ey.v);
    o.x0 = x0; o.y0 = y0; o.fx = fx; o.fy = fy;
    return o;
}

__device__ __forceinline__ bool is_valid(const WarpArgs& a, const GeoOut& g) { return g.in_n && g.e < (double)a.th; }

__global__ __launch_bounds__(WB) void warp_geo_fwd(WarpArgs a, const float* __restrict__ Dv, const float* __restrict__ Dn,
                                                   const float* __restrict__ camv, const float* __restrict__ camn, WarpWs w,
                                                   float* __restrict__ weight)
{
    __shared__ double s_sum[WB / 64];
    __shared__ int s_cnt[WB / 64];
    Cam cv, cn;
    load_cam(camv, cv);
    load_cam(camn, cn);
    const int HW = a.H * a.W;
    const int p = blockIdx.x * WB + threadIdx.x;
    double we = 0.0;
    int valid = 0;
    if (p < HW) {
        const int x = p % a.W, y = p / a.W;
        const GeoOut g = geo_pixel(a, cv, cn, Dn, x, y, Dv[p]);
        valid = is_valid(a, g);
        const double wt = valid ? 1.0 / exp(g.e) : 0.0;
        weight[p] = (float)wt;
        w.valid[p] = (uint8_t)valid;
        if (valid) we = wt * g.e;
    }
    for (int o = 32; o > 0; o >>= 1) {
        we += __shfl_xor(we, o, 64);
        valid += __shfl_xor(valid, o, 64);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_sum[wv] = we; s_cnt[wv] = valid; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int c = 0;
        for (int i = 0; i < WB / 64; ++i) { s += s_sum[i]; c += s_cnt[i]; }
        w.geo_part[blockIdx.x] = s;
        w.cnt_part[blockIdx.x] = c;
    }
}

// one workgroup: fixed-order sums of per-workgroup partials (thread t takes t, t + FIN, ...; then a tree)
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = FIN / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(FIN) void warp_geo_finalize(WarpArgs a, WarpWs w, int nbg, float* __restrict__ out_terms,
                                                         int32_t* __restrict__ out_counts)
{
    __shared__ double sd[FIN];
    __shared__ long long si[FIN];
    double s = 0.0;
    long long c = 0;
    for (int i = threadIdx.x; i < nbg; i += FIN) { s += w.geo_part[i]; c += w.cnt_part[i]; }
    s = block_sum(s, sd);
    c = block_sum(c, si);
    if (threadIdx.x == 0) {
        const int nv = (int)c;
        w.st[ST_NVALID] = nv;
        const int nsel = a.n_given >= 0 ? a.n_given : (nv < a.k ? nv : a.k);
        w.st[ST_NSEL] = nv > 0 ? nsel : 0;
        w.st[ST_TAKEALL] = (a.n_given < 0 && nv <= a.k) ? 1 : 0;
        w.st[ST_BIN] = 0; w.st[ST_REM] = a.k; w.st[ST_THRESH] = 0; w.st[ST_NKEEP] = 0;
        out_terms[0] = (nv > 0 && (a.flags & MRGS_WARP_GEO)) ? (float)((double)a.geo_w * s / (double)nv) : 0.f;
        out_terms[1] = out_terms[2] = out_terms[3] = 0.f;
        out_counts[0] = nv;
        out_counts[1] = w.st[ST_NSEL];
        out_counts[2] = 0;
        out_counts[3] = 0;
    }
}

// ---- sampler ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WB) void warp_sel_hist(WarpArgs a, WarpWs w, int pass)
{
    const int p = blockIdx.x * WB + threadIdx.x;
    if (p >= a.H * a.W || w.st[ST_TAKEALL] || !w.valid[p]) return;
    const uint32_t key = pixel_key((uint32_t)p, a.s0, a.s1);
    if (pass == 0) {
        atomicAdd(&w.hist[key >> 16], 1u);
    } else if ((int)(key >> 16) == w.st[ST_BIN]) {
        atomicAdd(&w.hist[NBINS + (key & 0xFFFFu)], 1u);
    }
}

// finds the bin holding the rank-th smallest key (rank = st[ST_REM], 1-based); pass 0: the high 16 bits, pass 1: the low 16 bits
__global__ __launch_bounds__(FIN) void warp_sel_scan(WarpWs w, int pass)
{
    __shared__ uint32_t s_wave[FIN / 64];
    if (w.st[ST_TAKEALL]) return;
    const uint32_t* hist = w.hist + pass * NBINS;
    constexpr int PER = NBINS / FIN;
    uint32_t mine = 0;
    for (int i = 0; i < PER; ++i) mine += hist[threadIdx.x * PER + i];
    const uint32_t rank = (uint32_t)w.st[ST_REM];        // read before the scan's barriers: the one thread below rewrites it
    uint32_t total;
    const uint32_t before = block_exclusive_scan<FIN>(mine, s_wave, total);
    if (before < rank && rank <= before + mine) {          // exactly one thread
        uint32_t c = before;
        for (int i = 0; i < PER; ++i) {
            const uint32_t hcount = hist[threadIdx.x * PER + i];
            if (rank <= c + hcount) {
                const int bin = threadIdx.x * PER + i;
                if (pass == 0) {
                    w.st[ST_BIN] = bin;
                    w.st[ST_REM] = (int)(rank - c);
                } else {
                    w.st[ST_THRESH] = (int)(((uint32_t)w.st[ST_BIN] << 16) | (uint32_t)bin);
                }
                break;
            }
            c += hcount;
        }
    }
}

__device__ __forceinline__ bool selected(const WarpArgs& a, const WarpWs& w, int p)
{
    if (!w.valid[p]) return false;
    if (w.st[ST_TAKEALL]) return true;
    return pixel_key((uint32_t)p, a.s0, a.s1) <= (uint32_t)w.st[ST_THRESH];
}

__global__ __launch_bounds__(WB) void warp_compact_count(WarpArgs a, WarpWs w)
{
    __shared__ int s_cnt[WB / 64];
    const int p = blockIdx.x * WB + threadIdx.x;
    const bool sel = p < a.H * a.W && selected(a, w, p);
    const uint64_t b = __ballot(sel);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) w.blk[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// exclusive scan of the per-workgroup counts, in place (one workgroup)
__global__ __launch_bounds__(FIN) void warp_compact_scan(WarpWs w, int nbg)
{
    __shared__ uint32_t s_wave[FIN / 64];
    uint32_t* blk = reinterpret_cast<uint32_t*>(w.blk);                  // counts: non-negative ints
    block_counts_exclusive_scan<FIN>(nbg, blk, blk, s_wave);
}

__global__ __launch_bounds__(WB) void warp_compact_write(WarpArgs a, WarpWs w)
{
    __shared__ int s_cnt[WB / 64];
    const int p = blockIdx.x * WB + threadIdx.x;
    const bool in = p < a.H * a.W;
    const bool sel = in && selected(a, w, p);
    const uint64_t b = __ballot(sel);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wv] = __popcll(b);
    __syncthreads();
    int off = w.blk[blockIdx.x];
    for (int i = 0; i < wv; ++i) off += s_cnt[i];
    off += __popcll(b & ((1ull << lane) - 1ull));
    if (!in) return;
    const bool put = sel && off < a.k;                  // (exactly k keys are <= the threshold: the guard never fires)
    if (put) w.samples[off] = p;
    w.slot[p] = put ? off : -1;
}

// samples given by the caller: slot map (cleared by the caller of this kernel) and the sample list
__global__ __launch_bounds__(WB) void warp_given_samples(WarpArgs a, WarpWs w, const int32_t* __restrict__ given)
{
    const int s = blockIdx.x * WB + threadIdx.x;
    if (s >= a.n_given) return;
    const int p = given[s];
    const bool in = p >= 0 && p < a.H * a.W;            // an index outside the image is read as pixel 0
    w.samples[s] = in ? p : 0;
    if (in) w.slot[p] = s;
}

// ---- patches ---------------------------------------------------------------------------------------------------------------------
struct Maps {
    const float *base_v, *metal_v, *rough_v, *base_n, *metal_n, *rough_n, *normal_v, *dist_v, *fg_v;
    const uint8_t* keep_v;
};

// H_s = K_n (R_rel - t_rel n^T / d) K_v^-1 (train_refnerf.py:562-586), row-major
__device__ __forceinline__ void homography(const WarpArgs& a, const Cam& cv, const Cam& cn, const Maps& m, int p, double* Hs)
{
    const size_t HW = (size_t)a.H * a.W;
    const double N[3] = {(double)m.normal_v[p], (double)m.normal_v[HW + p], (double)m.normal_v[2 * HW + p]};
    const double d = (double)m.dist_v[p];
    double n[3], Rr[3][3], t[3], M[3][3];
    for (int j = 0; j < 3; ++j) n[j] = N[0] * cv.Wm[0][j] + N[1] * cv.Wm[1][j] + N[2] * cv.Wm[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rr[i][j] = cn.Wm[0][i] * cv.Wm[0][j] + cn.Wm[1][i] * cv.Wm[1][j] + cn.Wm[2][i] * cv.Wm[2][j];
    for (int i = 0; i < 3; ++i) t[i] = -(Rr[i][0] * cv.Wm[3][0] + Rr[i][1] * cv.Wm[3][1] + Rr[i][2] * cv.Wm[3][2]) + cn.Wm[3][i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = Rr[i][j] - t[i] * n[j] / d;
    // K_n M
    double KM[3][3];
    for (int j = 0; j < 3; ++j) {
        KM[0][j] = a.fxn * M[0][j] + a.cxn * M[2][j];
        KM[1][j] = a.fyn * M[1][j] + a.cyn * M[2][j];
        KM[2][j] = M[2][j];
    }
    // (K_n M) K_v^-1, K_v^-1 = [[1/fx, 0, -cx/fx], [0, 1/fy, -cy/fy], [0, 0, 1]]
    for (int i = 0; i < 3; ++i) {
        Hs[i * 3 + 0] = KM[i][0] * (1.0 / a.fxv);
        Hs[i * 3 + 1] = KM[i][1] * (1.0 / a.fyv);
        Hs[i * 3 + 2] = KM[i][0] * (-a.cxv / a.fxv) + KM[i][1] * (-a.cyv / a.fyv) + KM[i][2];
    }
}

// bilinear footprint of the neighbour tap at pixel (tx, ty) of v (zeros padding, align_corners); ok = false: the tap samples zero
struct Foot {
    bool ok;
    int x0, y0;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ Foot nbr_foot(const WarpArgs& a, const double* Hs, int tx, int ty)
{
    Foot f;
    const double X = (double)tx, Y = (double)ty;
    const double gz = Hs[6] * X + Hs[7] * Y + Hs[8];
    const double gx = (Hs[0] * X + Hs[1] * Y + Hs[2]) / (gz + 1e-10);
    const double gy = (Hs[3] * X + Hs[4] * Y + Hs[5]) / (gz + 1e-10);
    // non-finite or far outside: every corner is out of bounds (grid_sample samples zero)
    f.ok = gx > -2.0 && gx < (double)a.W + 1.0 && gy > -2.0 && gy < (double)a.H + 1.0;
    f.x0 = f.y0 = 0;
    f.w00 = f.w01 = f.w10 = f.w11 = 0.f;
    if (!f.ok) return f;
    const double fx0 = floor(gx), fy0 = floor(gy);
    const double fx = gx - fx0, fy = gy - fy0;
    f.x0 = (int)fx0; f.y0 = (int)fy0;
    f.w00 = (float)((1.0 - fx) * (1.0 - fy));
    f.w01 = (float)(fx * (1.0 - fy));
    f.w10 = (float)((1.0 - fx) * fy);
    f.w11 = (float)(fx * fy);
    return f;
}

__device__ __forceinline__ bool inb(const WarpArgs& a, int x, int y) { return x >= 0 && y >= 0 && x < a.W && y < a.H; }

__device__ __forceinline__ float bil(const WarpArgs& a, const Foot& f, const float* __restrict__ img)
{
    if (!f.ok) return 0.f;
    float v = 0.f;
    if (inb(a, f.x0, f.y0)) v += f.w00 * img[(size_t)f.y0 * a.W + f.x0];
    if (inb(a, f.x0 + 1, f.y0)) v += f.w01 * img[(size_t)f.y0 * a.W + f.x0 + 1];
    if (inb(a, f.x0, f.y0 + 1)) v += f.w10 * img[(size_t)(f.y0 + 1) * a.W + f.x0];
    if (inb(a, f.x0 + 1, f.y0 + 1)) v += f.w11 * img[(size_t)(f.y0 + 1) * a.W + f.x0 + 1];
    return v;
}

__device__ __forceinline__ void scatter(const WarpArgs& a, const Foot& f, float* __restrict__ g, float v)
{
    if (!f.ok || v == 0.f) return;
    if (inb(a, f.x0, f.y0)) atomicAdd(&g[(size_t)f.y0 * a.W + f.x0], f.w00 * v);
    if (inb(a, f.x0 + 1, f.y0)) atomicAdd(&g[(size_t)f.y0 * a.W + f.x0 + 1], f.w01 * v);
    if (inb(a, f.x0, f.y0 + 1)) atomicAdd(&g[(size_t)(f.y0 + 1) * a.W + f.x0], f.w10 * v);
    if (inb(a, f.x0 + 1, f.y0 + 1)) atomicAdd(&g[(size_t)(f.y0 + 1) * a.W + f.x0 + 1], f.w11 * v);
}

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// L(d) of train_refnerf.py:640-644 and its derivative
__device__ __forceinline__ float Lf(float d) { return d < 0.2f ? 0.2f * (d / 0.2f) * (d / 0.2f) * (d / 0.2f) : d + (expf(5.f * (d - 0.2f)) - 1.f) / 5.f; }
__device__ __forceinline__ float dLf(float d) { return d < 0.2f ? 3.f * (d / 0.2f) * (d / 0.2f) : 1.f + expf(5.f * (d - 0.2f)); }

__global__ __launch_bounds__(WB) void warp_patch_fwd(WarpArgs a, WarpWs w, Maps m, const float* __restrict__ camv,
                                                     const float* __restrict__ camn, const float* __restrict__ weight)
{
    const int s = blockIdx.x * (WB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= w.st[ST_NSEL]) return;
    Cam cv, cn;
    load_cam(camv, cv);
    load_cam(camn, cn);
    const size_t HW = (size_t)a.H * a.W;
    const int p = w.samples[s];
    const int x = p % a.W, y = p / a.W;
    double Hs[9];
    homography(a, cv, cn, m, p, Hs);
    const bool tap = lane < a.P;
    const int side = 2 * a.h + 1;
    const int tx = x + (lane % side) - a.h, ty = y + (lane / side) - a.h;
    float sb = 0.f, sM = 0.f, sm1 = 0.f, sm2 = 0.f, sr1 = 0.f, sr2 = 0.f, fg = INFINITY;
    if (tap) {
        const bool vin = inb(a, tx, ty);
        const size_t q = vin ? (size_t)ty * a.W + tx : 0;
        const Foot f = nbr_foot(a, Hs, tx, ty);
        for (int c = 0; c < 3; ++c) {
            const float b = vin ? m.base_v[c * HW + q] : 0.f;
            sb += fabsf(b - bil(a, f, m.base_n + c * HW));
        }
        fg = vin ? m.fg_v[q] : 0.f;
        if (a.flags & MRGS_WARP_METALLIC) {
            const float mv = vin ? m.metal_v[q] : 0.f, mn = bil(a, f, m.metal_n);
            const float M = fmaxf(mn, mv);
            sM = M; sm1 = fabsf(mv - M); sm2 = fabsf(mn - M);
        }
        if (a.flags & MRGS_WARP_ROUGHNESS) {
            const float rv = vin ? m.rough_v[q] : 0.f, rn = bil(a, f, m.rough_n);
            const float mn = fminf(rn, rv);
            sr1 = fabsf(rv - mn); sr2 = fabsf(rn - mn);
        }
    }
    sb = wave_shfl_sum(sb); sM = wave_shfl_sum(sM); sm1 = wave_shfl_sum(sm1); sm2 = wave_shfl_sum(sm2); sr1 = wave_shfl_sum(sr1); sr2 = wave_shfl_sum(sr2); fg = wave_shfl_min(fg);
    if (lane < 9) w.homog[(size_t)s * 9 + lane] = Hs[lane];
    if (lane == 0) {
        const float P = (float)a.P, wt = weight[p];
        const bool keep = fg > 0.99f && (m.keep_v == nullptr || m.keep_v[p] != 0);
        const float vw = sM / P;
        const float tm = vw * (sm1 / P) * wt + vw * (sm2 / P) * wt;
        const float tr = (sr1 / P) * wt + (sr2 / P) * wt;
        w.terms[s] = (sb / P) * wt;
        w.terms[a.k + s] = keep ? Lf(tm) : 0.f;
        w.terms[2 * a.k + s] = keep ? Lf(tr) : 0.f;
        w.rec[s] = make_float4(wt, keep ? dLf(tm) * vw : 0.f, keep ? dLf(tr) : 0.f, keep ? 1.f : 0.f);
    }
}

__global__ __launch_bounds__(FIN) void warp_patch_finalize(WarpArgs a, WarpWs w, float* __restrict__ out_terms,
                                                           int32_t* __restrict__ out_counts)
{
    __shared__ double sd[FIN];
    const int ns = w.st[ST_NSEL];
    double b = 0.0, lm = 0.0, lr = 0.0, kp = 0.0;
    for (int i = threadIdx.x; i < ns; i += FIN) {
        b += w.terms[i];
        lm += w.terms[a.k + i];
        lr += w.terms[2 * a.k + i];
        kp += w.rec[i].w;
    }
    b = block_sum(b, sd);
    lm = block_sum(lm, sd);
    lr = block_sum(lr, sd);
    kp = block_sum(kp, sd);
    if (threadIdx.x == 0) {
        const int nkeep = (int)kp;
        w.st[ST_NKEEP] = nkeep;
        out_counts[2] = nkeep;
        if (w.st[ST_NVALID] == 0) return;                 // out_terms[1..3] stay 0 (warp_geo_finalize)
        out_terms[1] = (float)((double)a.base_w * b / (double)ns);
        // an empty keep set: mean of nothing, NaN as in the reference
        if (a.flags & MRGS_WARP_METALLIC) out_terms[2] = nkeep > 0 ? (float)((double)a.metal_w * lm / (double)nkeep) : __builtin_nanf("");
        if (a.flags & MRGS_WARP_ROUGHNESS) out_terms[3] = nkeep > 0 ? (float)((double)a.rough_w * lr / (double)nkeep) : __builtin_nanf("");
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WB) void warp_geo_bwd(WarpArgs a, const float* __restrict__ Dv, const float* __restrict__ Dn,
                                                   const float* __restrict__ camv, const float* __restrict__ camn, WarpWs w,
                                                   const float* __restrict__ weight, const float* __restrict__ g_terms,
                                                   float* __restrict__ g_dv, float* __restrict__ g_dn)
{
    const int p = blockIdx.x * WB + threadIdx.x;
    if (p >= a.H * a.W) return;
    const int nv = w.st[ST_NVALID];
    float gv = 0.f;
    if (w.valid[p] && nv > 0) {
        Cam cv, cn;
        load_cam(camv, cv);
        load_cam(camn, cn);
        const int x = p % a.W, y = p / a.W;
        const GeoOut g = geo_pixel(a, cv, cn, Dn, x, y, Dv[p]);
        const double c = (double)g_terms[0] * (double)a.geo_w * (double)weight[p] / (double)nv;
        if (g.e > 0.0) {
            const double da = (g.ex.v * g.ex.a + g.ey.v * g.ey.a) / g.e;
            const double db = (g.ex.v * g.ex.b + g.ey.v * g.ey.b) / g.e;
            gv = (float)(c * da);
            if (g_dn) {
                const float gz = (float)(c * db);
                const double fx = g.fx, fy = g.fy;
                if (g.x0 < a.W && g.y0 < a.H) atomicAdd(&g_dn[(size_t)g.y0 * a.W + g.x0], (float)((1.0 - fx) * (1.0 - fy)) * gz);
                if (g.x0 + 1 < a.W && g.y0 < a.H) atomicAdd(&g_dn[(size_t)g.y0 * a.W + g.x0 + 1], (float)(fx * (1.0 - fy)) * gz);
                if (g.x0 < a.W && g.y0 + 1 < a.H) atomicAdd(&g_dn[(size_t)(g.y0 + 1) * a.W + g.x0], (float)((1.0 - fx) * fy) * gz);
                if (g.x0 + 1 < a.W && g.y0 + 1 < a.H) atomicAdd(&g_dn[(size_t)(g.y0 + 1) * a.W + g.x0 + 1], (float)(fx * fy) * gz);
            }
        }
    }
    if (g_dv) g_dv[p] = gv;
}

struct GradMaps {
    float *base_v, *metal_v, *rough_v, *base_n, *metal_n, *rough_n;
};

// per-sample coefficients of dLoss/d|.| for the three terms
struct Coef {
    float cb, cm, cr;
};

__device__ __forceinline__ Coef sample_coef(const WarpArgs& a, const WarpWs& w, const float* __restrict__ g_terms, int s)
{
    const float4 r = w.rec[s];
    const float P = (float)a.P;
    const int ns = w.st[ST_NSEL], nk = w.st[ST_NKEEP];
    Coef c;
    c.cb = g_terms[1] * a.base_w / ((float)ns * P) * r.x;
    c.cm = (nk > 0 && (a.flags & MRGS_WARP_METALLIC)) ? g_terms[2] * a.metal_w / (float)nk * r.y * r.x / P : 0.f;
    c.cr = (nk > 0 && (a.flags & MRGS_WARP_ROUGHNESS)) ? g_terms[3] * a.rough_w / (float)nk * r.z * r.x / P : 0.f;
    return c;
}

// view maps: every pixel gathers from the samples whose patch covers it (fixed order over the offsets; no atomics)
__global__ __launch_bounds__(WB) void warp_view_gather(WarpArgs a, WarpWs w, Maps m, const float* __restrict__ g_terms, GradMaps g)
{
    const int q = blockIdx.x * WB + threadIdx.x;
    if (q >= a.H * a.W) return;
    const size_t HW = (size_t)a.H * a.W;
    const int x = q % a.W, y = q / a.W;
    float gb[3] = {0.f, 0.f, 0.f}, gm = 0.f, gr = 0.f;
    if (w.st[ST_NVALID] > 0) {
        const float b[3] = {m.base_v[q], m.base_v[HW + q], m.base_v[2 * HW + q]};
        const float mv = (a.flags & MRGS_WARP_METALLIC) ? m.metal_v[q] : 0.f;
        const float rv = (a.flags & MRGS_WARP_ROUGHNESS) ? m.rough_v[q] : 0.f;
        for (int oy = -a.h; oy <= a.h; ++oy) {
            for (int ox = -a.h; ox <= a.h; ++ox) {
                const int cx = x - ox, cy = y - oy;
                if (!inb(a, cx, cy)) continue;
                const int s = w.slot[(size_t)cy * a.W + cx];
                if (s < 0) continue;
                double Hs[9];
                for (int i = 0; i < 9; ++i) Hs[i] = w.homog[(size_t)s * 9 + i];
                const Foot f = nbr_foot(a, Hs, x, y);
                const Coef c = sample_coef(a, w, g_terms, s);
                for (int ch = 0; ch < 3; ++ch) gb[ch] += c.cb * sgn(b[ch] - bil(a, f, m.base_n + ch * HW));
                if (c.cm != 0.f) {
                    const float M = fmaxf(bil(a, f, m.metal_n), mv);
                    gm += c.cm * sgn(mv - M);
                }
                if (c.cr != 0.f) {
                    const float mn = fminf(bil(a, f, m.rough_n), rv);
                    gr += c.cr * sgn(rv - mn);
                }
            }
        }
    }
    if (g.base_v) { g.base_v[q] = gb[0]; g.base_v[HW + q] = gb[1]; g.base_v[2 * HW + q] = gb[2]; }
    if (g.metal_v) g.metal_v[q] = gm;
    if (g.rough_v) g.rough_v[q] = gr;
}

// neighbour maps: the bilinear corners of every tap (atomics into buffers the caller cleared)
__global__ __launch_bounds__(WB) void warp_nbr_scatter(WarpArgs a, WarpWs w, Maps m, const float* __restrict__ g_terms, GradMaps g)
{
    const int s = blockIdx.x * (WB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= w.st[ST_NSEL] || w.st[ST_NVALID] == 0 || lane >= a.P) return;
    const size_t HW = (size_t)a.H * a.W;
    const int p = w.samples[s];
    const int x = p % a.W, y = p / a.W;
    double Hs[9];
    for (int i = 0; i < 9; ++i) Hs[i] = w.homog[(size_t)s * 9 + i];
    const int side = 2 * a.h + 1;
    const int tx = x + (lane % side) - a.h, ty = y + (lane / side) - a.h;
    const Foot f = nbr_foot(a, Hs, tx, ty);
    if (!f.ok) return;
    const bool vin = inb(a, tx, ty);
    const size_t q = vin ? (size_t)ty * a.W + tx : 0;
    const Coef c = sample_coef(a, w, g_terms, s);
    if (g.base_n)
        for (int ch = 0; ch < 3; ++ch) {
            const float b = vin ? m.base_v[ch * HW + q] : 0.f;
            scatter(a, f, g.base_n + ch * HW, -c.cb * sgn(b - bil(a, f, m.base_n + ch * HW)));
        }
    if (g.metal_n && c.cm != 0.f) {
        const float mv = vin ? m.metal_v[q] : 0.f, mn = bil(a, f, m.metal_n);
        scatter(a, f, g.metal_n, c.cm * sgn(mn - fmaxf(mn, mv)));
    }
    if (g.rough_n && c.cr != 0.f) {
        const float rv = vin ? m.rough_v[q] : 0.f, rn = bil(a, f, m.rough_n);
        scatter(a, f, g.rough_n, c.cr * sgn(rn - fminf(rn, rv)));
    }
}

uint32_t host_fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

int make_args(const MrgsWarpConfig* cfg, WarpArgs& a)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsWarpConfig)) return MRGS_E_BAD_ARG;
    if (cfg->H <= 0 || cfg->W <= 0 || (int64_t)cfg->H * cfg->W >= ((int64_t)1 << 30)) return MRGS_E_BAD_ARG;
    if (cfg->sample_num <= 0 || cfg->patch_half < 1 || cfg->patch_half > 3) return MRGS_E_BAD_ARG;
    if (cfg->n_given < -1 || cfg->n_given > cfg->sample_num) return MRGS_E_BAD_ARG;
    if (cfg->flags & ~(uint32_t)(MRGS_WARP_GEO | MRGS_WARP_MATERIAL | MRGS_WARP_METALLIC | MRGS_WARP_ROUGHNESS)) return MRGS_E_BAD_ARG;
    if ((cfg->flags & (MRGS_WARP_METALLIC | MRGS_WARP_ROUGHNESS)) && !(cfg->flags & MRGS_WARP_MATERIAL)) return MRGS_E_BAD_ARG;
    const float f[8] = {cfg->fx_v, cfg->fy_v, cfg->cx_v, cfg->cy_v, cfg->fx_n, cfg->fy_n, cfg->cx_n, cfg->cy_n};
    for (int i = 0; i < 8; ++i)
        if (!(f[i] == f[i]) || (i % 4 < 2 && !(f[i] > 0.f))) return MRGS_E_BAD_ARG;
    a.H = cfg->H; a.W = cfg->W; a.k = cfg->sample_num; a.h = cfg->patch_half; a.P = (2 * a.h + 1) * (2 * a.h + 1);
    a.n_given = cfg->n_given; a.flags = cfg->flags;
    a.s0 = host_fmix32(cfg->seed_lo ^ 0x9e3779b9u);
    a.s1 = host_fmix32(cfg->seed_hi + 0x7f4a7c15u + a.s0);
    a.fxv = cfg->fx_v; a.fyv = cfg->fy_v; a.cxv = cfg->cx_v; a.cyv = cfg->cy_v;
    a.fxn = cfg->fx_n; a.fyn = cfg->fy_n; a.cxn = cfg->cx_n; a.cyn = cfg->cy_n;
    a.th = cfg->pixel_noise_th; a.geo_w = cfg->geo_weight; a.base_w = cfg->base_weight; a.metal_w = cfg->metallic_weight;
    a.rough_w = cfg->roughness_weight;
    return MRGS_OK;
}

Maps make_maps(const MrgsWarpMaps* mp)
{
    Maps m;
    m.base_v = mp->base_v; m.metal_v = mp->metal_v; m.rough_v = mp->rough_v;
    m.base_n = mp->base_n; m.metal_n = mp->metal_n; m.rough_n = mp->rough_n;
    m.normal_v = mp->normal_v; m.dist_v = mp->distance_v; m.fg_v = mp->fg_v; m.keep_v = mp->keep_v;
    return m;
}

int check_maps(const WarpArgs& a, const MrgsWarpMaps* mp)
{
    if (!mp || !mp->depth_v || !mp->depth_n || !mp->cam_v || !mp->cam_n) return MRGS_E_BAD_ARG;
    if (a.flags & MRGS_WARP_MATERIAL)
        if (!mp->normal_v || !mp->distance_v || !mp->base_v || !mp->base_n || !mp->fg_v) return MRGS_E_BAD_ARG;
    if ((a.flags & MRGS_WARP_METALLIC) && (!mp->metal_v || !mp->metal_n)) return MRGS_E_BAD_ARG;
    if ((a.flags & MRGS_WARP_ROUGHNESS) && (!mp->rough_v || !mp->rough_n)) return MRGS_E_BAD_ARG;
    return MRGS_OK;
}

// the sample list and the slot map of w: the caller's samples (n_given >= 0) or the draw over w.valid; w.st holds warp_geo_finalize's words
int draw_samples(const WarpArgs& a, const WarpWs& w, int32_t* samples, hipStream_t st)
{
    const int HW = a.H * a.W, nbg = (HW + WB - 1) / WB;
    if (a.n_given >= 0) {
        MRGS_HIP_TRY(hipMemsetAsync(w.slot, 0xFF, (size_t)HW * 4, st));
        if (a.n_given > 0) warp_given_samples<<<(a.n_given + WB - 1) / WB, WB, 0, st>>>(a, w, samples);
    } else {
        MRGS_HIP_TRY(hipMemsetAsync(w.hist, 0, 2 * (size_t)NBINS * 4, st));
        warp_sel_hist<<<nbg, WB, 0, st>>>(a, w, 0);
        warp_sel_scan<<<1, FIN, 0, st>>>(w, 0);
        warp_sel_hist<<<nbg, WB, 0, st>>>(a, w, 1);
        warp_sel_scan<<<1, FIN, 0, st>>>(w, 1);
        warp_compact_count<<<nbg, WB, 0, st>>>(a, w);
        warp_compact_scan<<<1, FIN, 0, st>>>(w, nbg);
        warp_compact_write<<<nbg, WB, 0, st>>>(a, w);
        if (samples) MRGS_HIP_TRY(hipMemcpyAsync(samples, w.samples, (size_t)a.k * 4, hipMemcpyDeviceToDevice, st));
    }
    return MRGS_OK;
}

}   // namespace

extern "C" size_t mrgs_warp_loss_ws_bytes(int32_t H, int32_t W, int32_t sample_num, int32_t patch_half)
{
    if (H <= 0 || W <= 0 || sample_num <= 0 || patch_half < 1 || patch_half > 3) return 0;
    return ws_layout(H, W, sample_num, nullptr, nullptr);
}

extern "C" int mrgs_warp_loss_forward(const MrgsWarpConfig* cfg, const MrgsWarpMaps* maps, int32_t* samples, void* ws, size_t ws_bytes,
                                      float* weight_map, float* out_terms, int32_t* out_counts, void* stream)
{
    WarpArgs a;
    int rc = make_args(cfg, a);
    if (rc) return rc;
    if ((rc = check_maps(a, maps))) return rc;
    if (!ws || !weight_map || !out_terms || !out_counts) return MRGS_E_BAD_ARG;
    if (a.n_given >= 0 && a.n_given > 0 && !samples) return MRGS_E_BAD_ARG;
    if (ws_bytes < ws_layout(a.H, a.W, a.k, nullptr, nullptr)) return MRGS_E_WORKSPACE;
    WarpWs w;
    ws_layout(a.H, a.W, a.k, &w, (char*)ws);
    hipStream_t st = (hipStream_t)stream;
    const int HW = a.H * a.W, nbg = (HW + WB - 1) / WB;
    warp_geo_fwd<<<nbg, WB, 0, st>>>(a, maps->depth_v, maps->depth_n, maps->cam_v, maps->cam_n, w, weight_map);
    warp_geo_finalize<<<1, FIN, 0, st>>>(a, w, nbg, out_terms, out_counts);
    if (!(a.flags & MRGS_WARP_MATERIAL)) return MRGS_LAUNCH_STATUS();
    if ((rc = draw_samples(a, w, samples, st))) return rc;
    const Maps m = make_maps(maps);
    const int ns_max = a.n_given >= 0 ? a.n_given : a.k;
    if (ns_max > 0) warp_patch_fwd<<<(ns_max + WB / 64 - 1) / (WB / 64), WB, 0, st>>>(a, w, m, maps->cam_v, maps->cam_n, weight_map);
    warp_patch_finalize<<<1, FIN, 0, st>>>(a, w, out_terms, out_counts);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_warp_loss_backward(const MrgsWarpConfig* cfg, const MrgsWarpMaps* maps, const void* ws, const float* weight_map,
                                       const float* g_terms, float* g_depth_v, float* g_depth_n, float* g_base_v, float* g_metal_v,
                                       float* g_rough_v, float* g_base_n, float* g_metal_n, float* g_rough_n, void* stream)
{
    WarpArgs a;
    int rc = make_args(cfg, a);
    if (rc) return rc;
    if ((rc = check_maps(a, maps))) return rc;
    if (!ws || !weight_map || !g_terms) return MRGS_E_BAD_ARG;
    WarpWs w;
    ws_layout(a.H, a.W, a.k, &w, (char*)ws);
    hipStream_t st = (hipStream_t)stream;
    const size_t HW = (size_t)a.H * a.W;
    const int nbg = (int)((HW + WB - 1) / WB);
    if (g_depth_n) MRGS_HIP_TRY(hipMemsetAsync(g_depth_n, 0, HW * 4, st));
    if ((g_depth_v || g_depth_n) && (a.flags & MRGS_WARP_GEO))
        warp_geo_bwd<<<nbg, WB, 0, st>>>(a, maps->depth_v, maps->depth_n, maps->cam_v, maps->cam_n, w, weight_map, g_terms, g_depth_v, g_depth_n);
    else if (g_depth_v)
        MRGS_HIP_TRY(hipMemsetAsync(g_depth_v, 0, HW * 4, st));
    GradMaps g{g_base_v, (a.flags & MRGS_WARP_METALLIC) ? g_metal_v : nullptr, (a.flags & MRGS_WARP_ROUGHNESS) ? g_rough_v : nullptr,
               g_base_n, (a.flags & MRGS_WARP_METALLIC) ? g_metal_n : nullptr, (a.flags & MRGS_WARP_ROUGHNESS) ? g_rough_n : nullptr};
    float* outs[6] = {g_base_v, g_metal_v, g_rough_v, g_base_n, g_metal_n, g_rough_n};
    const size_t chans[6] = {3, 1, 1, 3, 1, 1};
    float* used[6] = {g.base_v, g.metal_v, g.rough_v, nullptr, nullptr, nullptr};
    bool material = (a.flags & MRGS_WARP_MATERIAL) != 0;
    // view maps the gather does not write, and every neighbour map (the scatter accumulates): cleared
    for (int i = 0; i < 6; ++i)
        if (outs[i] && (!material || i >= 3 || !used[i]))
            MRGS_HIP_TRY(hipMemsetAsync(outs[i], 0, chans[i] * HW * 4, st));
    if (material) {
        const Maps m = make_maps(maps);
        if (g.base_v || g.metal_v || g.rough_v) warp_view_gather<<<nbg, WB, 0, st>>>(a, w, m, g_terms, g);
        const int ns_max = a.n_given >= 0 ? a.n_given : a.k;
        if ((g.base_n || g.metal_n || g.rough_n) && ns_max > 0)
            warp_nbr_scatter<<<(ns_max + WB / 64 - 1) / (WB / 64), WB, 0, st>>>(a, w, m, g_terms, g);
    }
    return MRGS_LAUNCH_STATUS();
}

// ---- grey-image patch NCC (get_consistency_loss2 over lncc; train_refreal.py:358-395, utils/loss_utils.py:230-265) -----------------
// The term of the multi-view loss whose gradient goes through the plane homography: it trains rend_normal and rend_distance of the view.
//   warp_ncc_fwd        one 64-lane wave per sample, one lane per tap: the view's grey tap r at its integer texel, the neighbour's q through
//                       the homography.  A tap position depends on (n, d) through the one scalar s = (n . K_v^-1 X) / d: H X = A - B s with
//                       B = K_n t_rel the same for every tap, so each lane carries dq/ds and the wave reduces the forward-mode derivative
//                       d ncc / d (rend_normal, rend_distance) next to the value.  Double throughout: the literal lncc sums cancel on
//                       low-contrast patches (var_r var_q next to the 1e-8 of the denominator), so the centred sums are taken instead.
//   warp_ncc_finalize   one workgroup: the used samples in a fixed order -> the scalar and the counts.
//   warp_ncc_bwd        per pixel of the view: the sample that owns it (slot map) scaled by the upstream gradient; no atomics.
namespace {

constexpr int ST_NUSED = 7;              // the NCC workspace's own state word (the other words are a copy of WarpWs::st)

struct NccWs {
    int32_t* st;                         // copy of the material call's state, + ST_NUSED
    uint32_t* hist;                      // the sampler's scratch when the material call drew nothing
    int32_t* blk;
    int32_t* slot;
    int32_t* samples;
    double* val;                         // [k] ncc_s w_s on used samples, 0 elsewhere
    float4* dval;                        // [k] w_s d ncc_s / d (N_x, N_y, N_z, d) on used samples, 0 elsewhere
    uint8_t* use;                        // [k]
};

size_t ncc_layout(int H, int W, int k, NccWs* n, char* base)
{
    const size_t HW = (size_t)H * W, nbg = (HW + WB - 1) / WB;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return base ? base + at : nullptr; };
    char* st = take(ST_WORDS * 4);
    char* hist = take(2 * (size_t)NBINS * 4);
    char* bk = take(nbg * 4);
    char* sl = take(HW * 4);
    char* sa = take((size_t)k * 4);
    char* va = take((size_t)k * 8);
    char* dv = take((size_t)k * 16);
    char* us = take((size_t)k);
    if (n) {
        n->st = (int32_t*)st; n->hist = (uint32_t*)hist; n->blk = (int32_t*)bk; n->slot = (int32_t*)sl; n->samples = (int32_t*)sa;
        n->val = (double*)va; n->dval = (float4*)dv; n->use = (uint8_t*)us;
    }
    return o;
}

struct NccIn {
    const float *normal_v, *dist_v, *metal_v, *metal_n, *grey_v, *grey_n, *camv, *camn, *weight;
    const int32_t* samples;
    const double* homog;                 // the material call's H_s, or nullptr (computed here)
};

__global__ __launch_bounds__(WB) void warp_ncc_fwd(WarpArgs a, NccIn in, NccWs n, float* __restrict__ ref_weight,
                                                   float* __restrict__ out_ncc, uint8_t* __restrict__ out_use)
{
    const int s = blockIdx.x * (WB / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= n.st[ST_NSEL]) return;
    Cam cv, cn;
    load_cam(in.camv, cv);
    load_cam(in.camn, cn);
    const size_t HW = (size_t)a.H * a.W;
    const int p = in.samples[s];
    const int x = p % a.W, y = p / a.W;
    double Hs[9];
    if (in.homog) {
        for (int i = 0; i < 9; ++i) Hs[i] = in.homog[(size_t)s * 9 + i];
    } else {
        Maps m{};
        m.normal_v = in.normal_v; m.dist_v = in.dist_v;
        homography(a, cv, cn, m, p, Hs);
    }
    // s_tap = (nc . r) / d with r = K_v^-1 X; H X = A - B s_tap, B = K_n t_rel
    const double N[3] = {(double)in.normal_v[p], (double)in.normal_v[HW + p], (double)in.normal_v[2 * HW + p]};
    const double d = (double)in.dist_v[p];
    double nc[3], t[3];
    for (int j = 0; j < 3; ++j) nc[j] = N[0] * cv.Wm[0][j] + N[1] * cv.Wm[1][j] + N[2] * cv.Wm[2][j];
    for (int i = 0; i < 3; ++i) {
        double ti = cn.Wm[3][i];
        for (int j = 0; j < 3; ++j) {
            const double Rij = cn.Wm[0][i] * cv.Wm[0][j] + cn.Wm[1][i] * cv.Wm[1][j] + cn.Wm[2][i] * cv.Wm[2][j];
            ti -= Rij * cv.Wm[3][j];
        }
        t[i] = ti;
    }
    const double Bx = a.fxn * t[0] + a.cxn * t[2], By = a.fyn * t[1] + a.cyn * t[2], Bz = t[2];
    const bool tap = lane < a.P;
    const int side = 2 * a.h + 1;
    const int tx = x + (lane % side) - a.h, ty = y + (lane / side) - a.h;
    double r = 0.0, q = 0.0, mv = 0.0, mn = 0.0, dq = 0.0;       // dq = dq / ds_tap
    double e[4] = {0.0, 0.0, 0.0, 0.0};                         // ds_tap / d (N_x, N_y, N_z, d)
    bool ok = false;
    if (tap) {
        if (inb(a, tx, ty)) {
            r = (double)in.grey_v[(size_t)ty * a.W + tx];
            mv = (double)in.metal_v[(size_t)ty * a.W + tx];
        }
        const double X = (double)tx, Y = (double)ty;
        const double gz = Hs[6] * X + Hs[7] * Y + Hs[8];
        const double den = gz + 1e-10;
        const double Gx = Hs[0] * X + Hs[1] * Y + Hs[2], Gy = Hs[3] * X + Hs[4] * Y + Hs[5];
        const double gx = Gx / den, gy = Gy / den;
        ok = gx > -2.0 && gx < (double)a.W + 1.0 && gy > -2.0 && gy < (double)a.H + 1.0;
        if (ok) {
            const double fx0 = floor(gx), fy0 = floor(gy);
            const double fx = gx - fx0, fy = gy - fy0;
            const int x0 = (int)fx0, y0 = (int)fy0;
            const bool b00 = inb(a, x0, y0), b01 = inb(a, x0 + 1, y0), b10 = inb(a, x0, y0 + 1), b11 = inb(a, x0 + 1, y0 + 1);
            const size_t i00 = (size_t)y0 * a.W + x0;            // (only dereferenced where the corner is inside)
            auto corner = [&](const float* __restrict__ img, double& v00, double& v01, double& v10, double& v11) {
                v00 = b00 ? (double)img[i00] : 0.0;
                v01 = b01 ? (double)img[i00 + 1] : 0.0;
                v10 = b10 ? (double)img[i00 + a.W] : 0.0;
                v11 = b11 ? (double)img[i00 + a.W + 1] : 0.0;
            };
            double v00, v01, v10, v11;
            corner(in.grey_n, v00, v01, v10, v11);
            q = v00 * ((1.0 - fx) * (1.0 - fy)) + v01 * (fx * (1.0 - fy)) + v10 * ((1.0 - fx) * fy) + v11 * (fx * fy);
            const double qx = (v01 - v00) * (1.0 - fy) + (v11 - v10) * fy;
            const double qy = (v10 - v00) * (1.0 - fx) + (v11 - v01) * fx;
            const double dgx = (Gx * Bz - Bx * den) / (den * den), dgy = (Gy * Bz - By * den) / (den * den);
            dq = qx * dgx + qy * dgy;
            corner(in.metal_n, v00, v01, v10, v11);
            mn = v00 * ((1.0 - fx) * (1.0 - fy)) + v01 * (fx * (1.0 - fy)) + v10 * ((1.0 - fx) * fy) + v11 * (fx * fy);
            const double rr[3] = {(X - a.cxv) / a.fxv, (Y - a.cyv) / a.fyv, 1.0};
            for (int i = 0; i < 3; ++i) e[i] = (cv.Wm[i][0] * rr[0] + cv.Wm[i][1] * rr[1] + cv.Wm[i][2] * rr[2]) / d;
            e[3] = -(nc[0] * rr[0] + nc[1] * rr[1] + nc[2] * rr[2]) / (d * d);
        }
    }
    const double P = (double)a.P;
    const double rbar = wave_shfl_sum(r) / P, qbar = wave_shfl_sum(q) / P, m_s = wave_shfl_sum(mv) / P + wave_shfl_sum(mn) / P;
    const double rc = tap ? r - rbar : 0.0, qc = tap ? q - qbar : 0.0;
    const double cross = wave_shfl_sum(rc * qc), var_r = wave_shfl_sum(rc * rc), var_q = wave_shfl_sum(qc * qc);
    const double D = var_r * var_q + 1e-8;
    const double raw = 1.0 - cross * cross / D;
    const double ncc = raw < 0.0 ? 0.0 : (raw > 2.0 ? 2.0 : raw);
    const bool use = ncc < 0.9 && m_s < 0.4;
    const float wt = in.weight[p];
    // d ncc / dq_p = -(2 cross rc_p / D - 2 cross^2 var_r qc_p / D^2); nothing passes the clamp outside [0, 2]
    const double al_ = 2.0 * cross / D, be_ = 2.0 * cross * cross * var_r / (D * D);
    const double c = (ok && use && raw >= 0.0 && raw <= 2.0) ? -(al_ * rc - be_ * qc) * dq : 0.0;
    double g[4];
    for (int i = 0; i < 4; ++i) g[i] = wave_shfl_sum(c != 0.0 ? c * e[i] : 0.0);
    if (lane == 0) {
        n.val[s] = use ? ncc * (double)wt : 0.0;
        n.use[s] = (uint8_t)use;
        n.dval[s] = use ? make_float4((float)((double)wt * g[0]), (float)((double)wt * g[1]), (float)((double)wt * g[2]), (float)((double)wt * g[3]))
                        : make_float4(0.f, 0.f, 0.f, 0.f);
        const double rw = 1.0 - m_s / 2.0;
        ref_weight[p] = rw < 0.9 ? 0.f : (float)rw;
        if (out_ncc) out_ncc[s] = (float)ncc;
        if (out_use) out_use[s] = (uint8_t)use;
    }
}

__global__ __launch_bounds__(FIN) void warp_ncc_finalize(NccWs n, float ncc_w, float* __restrict__ out_term, int32_t* __restrict__ out_counts)
{
    __shared__ double sd[FIN];
    __shared__ long long si[FIN];
    const int ns = n.st[ST_NSEL];
    double v = 0.0;
    long long c = 0;
    for (int i = threadIdx.x; i < ns; i += FIN) { v += n.val[i]; c += n.use[i]; }
    v = block_sum(v, sd);
    c = block_sum(c, si);
    if (threadIdx.x == 0) {
        const int nu = n.st[ST_NVALID] > 0 ? (int)c : 0;
        n.st[ST_NUSED] = nu;
        out_term[0] = nu > 0 ? (float)((double)ncc_w * v / (double)nu) : 0.f;
        out_counts[0] = ns;
        out_counts[1] = nu;
    }
}

__global__ __launch_bounds__(WB) void warp_ncc_bwd(int HW, const int32_t* __restrict__ slot, NccWs n, float ncc_w, const float* __restrict__ g_term,
                                                   float* __restrict__ g_normal, float* __restrict__ g_dist)
{
    const int p = blockIdx.x * WB + threadIdx.x;
    if (p >= HW) return;
    const int s = slot[p], nu = n.st[ST_NUSED];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s >= 0 && nu > 0 && n.use[s]) {
        const double c = (double)g_term[0] * (double)ncc_w / (double)nu;
        const float4 dv = n.dval[s];
        o = make_float4((float)(c * dv.x), (float)(c * dv.y), (float)(c * dv.z), (float)(c * dv.w));
    }
    if (g_normal) { g_normal[p] = o.x; g_normal[(size_t)HW + p] = o.y; g_normal[2 * (size_t)HW + p] = o.z; }
    if (g_dist) g_dist[p] = o.w;
}

// the NCC calls accept the configuration of the material call they follow
int ncc_args(const MrgsWarpConfig* cfg, const MrgsWarpMaps* mp, float ncc_w, WarpArgs& a)
{
    if (int rc = make_args(cfg, a)) return rc;
    if (!(ncc_w == ncc_w)) return MRGS_E_BAD_ARG;
    if (mp && (!mp->cam_v || !mp->cam_n || !mp->normal_v || !mp->distance_v || !mp->metal_v || !mp->metal_n)) return MRGS_E_BAD_ARG;
    return MRGS_OK;
}

}   // namespace

extern "C" size_t mrgs_warp_ncc_ws_bytes(int32_t H, int32_t W, int32_t sample_num, int32_t patch_half)
{
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 30) || sample_num <= 0 || patch_half < 1 || patch_half > 3) return 0;
    return ncc_layout(H, W, sample_num, nullptr, nullptr);
}

extern "C" int mrgs_warp_ncc_forward(const MrgsWarpConfig* cfg, const MrgsWarpMaps* maps, const float* grey_v, const float* grey_n,
                                     const float* weight_map, const void* warp_ws, size_t warp_ws_bytes, int32_t* samples, void* ws,
                                     size_t ws_bytes, float ncc_weight, float* out_term, int32_t* out_counts, float* ref_weight_map,
                                     float* out_ncc, uint8_t* out_use, void* stream)
{
    WarpArgs a;
    if (!maps) return MRGS_E_BAD_ARG;
    if (int rc = ncc_args(cfg, maps, ncc_weight, a)) return rc;
    if (!grey_v || !grey_n || !weight_map || !warp_ws || !ws || !out_term || !out_counts || !ref_weight_map) return MRGS_E_BAD_ARG;
    if (a.n_given > 0 && !(a.flags & MRGS_WARP_MATERIAL) && !samples) return MRGS_E_BAD_ARG;
    if (warp_ws_bytes < ws_layout(a.H, a.W, a.k, nullptr, nullptr) || ws_bytes < ncc_layout(a.H, a.W, a.k, nullptr, nullptr))
        return MRGS_E_WORKSPACE;
    WarpWs w;
    NccWs n;
    ws_layout(a.H, a.W, a.k, &w, (char*)warp_ws);
    ncc_layout(a.H, a.W, a.k, &n, (char*)ws);
    hipStream_t st = (hipStream_t)stream;
    const int HW = a.H * a.W;
    MRGS_HIP_TRY(hipMemcpyAsync(n.st, w.st, ST_WORDS * 4, hipMemcpyDeviceToDevice, st));
    MRGS_HIP_TRY(hipMemsetAsync(ref_weight_map, 0, (size_t)HW * 4, st));
    NccIn in{maps->normal_v, maps->distance_v, maps->metal_v, maps->metal_n, grey_v, grey_n, maps->cam_v, maps->cam_n, weight_map,
             w.samples, w.homog};
    if (!(a.flags & MRGS_WARP_MATERIAL)) {
        // the material call drew nothing: the same sampler on its valid map, into this workspace (equal seed and valid set: equal draw)
        WarpWs d = w;
        d.st = n.st; d.hist = n.hist; d.blk = n.blk; d.slot = n.slot; d.samples = n.samples;
        const int rcd = draw_samples(a, d, samples, st);
        if (rcd) return rcd;
        in.samples = n.samples;
        in.homog = nullptr;
    }
    const int ns_max = a.n_given >= 0 ? a.n_given : a.k;
    if (ns_max > 0) warp_ncc_fwd<<<(ns_max + WB / 64 - 1) / (WB / 64), WB, 0, st>>>(a, in, n, ref_weight_map, out_ncc, out_use);
    warp_ncc_finalize<<<1, FIN, 0, st>>>(n, ncc_weight, out_term, out_counts);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_warp_ncc_backward(const MrgsWarpConfig* cfg, const void* warp_ws, const void* ws, float ncc_weight, const float* g_term,
                                      float* g_normal_v, float* g_distance_v, void* stream)
{
    WarpArgs a;
    if (int rc = ncc_args(cfg, nullptr, ncc_weight, a)) return rc;
    if (!warp_ws || !ws || !g_term) return MRGS_E_BAD_ARG;
    if (!g_normal_v && !g_distance_v) return MRGS_OK;
    WarpWs w;
    NccWs n;
    ws_layout(a.H, a.W, a.k, &w, (char*)warp_ws);
    ncc_layout(a.H, a.W, a.k, &n, (char*)ws);
    const int HW = a.H * a.W;
    const int32_t* slot = (a.flags & MRGS_WARP_MATERIAL) ? w.slot : n.slot;
    warp_ncc_bwd<<<(HW + WB - 1) / WB, WB, 0, (hipStream_t)stream>>>(HW, slot, n, ncc_weight, g_term, g_normal_v, g_distance_v);
    return MRGS_LAUNCH_STATUS();
}

// ---- multi-view reflection score (calc_ref_score, train_refreal.py:782-1001) ---------------------------------------------------------
// Dense, where the kernels above work on a sample list: every pixel of the view against all of its K neighbours, (2h+1)^2 <= 81 taps.
//   ref_score_fwd       one 64-lane wave per 8x8 pixel block, one pixel per lane.  The view's (8+2h)^2 x 3 anchor tile sits in LDS.
//                       Neighbours outside, taps inside: geo_pixel decides validity, a ballot skips a neighbour no lane is valid for
//                       (background blocks cost the geometry only), then every valid lane walks its patch through its own homography
//                       (homography, nbr_foot and bil above: positions in double, colours in fp32).  |s - a| is summed per tap row,
//                       the rows per neighbour, the neighbours per pixel, all in fp32 and in a fixed order: no atomics, no workspace.
namespace {

constexpr int RS_B = 8;                  // pixel block side: 8 x 8 = one wave
constexpr int RS_TS = RS_B + 2 * 4;      // anchor tile side at the largest patch
constexpr int RS_LD = 24;                // tile row stride in floats: rows 0..3 (and 4..7) of a half wave fall on distinct banks

struct RefArgs {
    int H, W, h, K;
    double fxv, fyv, cxv, cyv;
    float th;
};

__global__ __launch_bounds__(64) void ref_score_fwd(RefArgs r, const float* __restrict__ Dv, const float* __restrict__ Nv,
                                                    const float* __restrict__ dist_v, const float* __restrict__ img_v,
                                                    const float* __restrict__ camv, const MrgsRefScoreNeighbour* __restrict__ nbrs,
                                                    float* __restrict__ score, int32_t* __restrict__ count)
{
    __shared__ float tile[3][RS_TS][RS_LD];
    const int lane = threadIdx.x;
    const int lx = lane & (RS_B - 1), ly = lane >> 3;
    const int nbx = (r.W + RS_B - 1) / RS_B;
    const int bx0 = (int)(blockIdx.x % nbx) * RS_B, by0 = (int)(blockIdx.x / nbx) * RS_B;
    const int x = bx0 + lx, y = by0 + ly;
    const size_t HW = (size_t)r.H * r.W;
    const int side = 2 * r.h + 1, ts = RS_B + 2 * r.h;
    // the anchor tile: image_v at the integer texels around the block, zero outside the image
    for (int i = lane; i < 3 * ts * ts; i += 64) {
        const int c = i / (ts * ts), q = i - c * ts * ts;
        const int ty = q / ts, tx = q - ty * ts;
        const int gx = bx0 - r.h + tx, gy = by0 - r.h + ty;
        const bool in = gx >= 0 && gy >= 0 && gx < r.W && gy < r.H;
        tile[c][ty][tx] = in ? img_v[c * HW + (size_t)gy * r.W + gx] : 0.f;
    }
    __syncthreads();
    const bool in = x < r.W && y < r.H;
    const int p = in ? y * r.W + x : 0;
    const float dv = in ? Dv[p] : 0.f;
    WarpArgs a{};
    a.H = r.H; a.W = r.W; a.h = r.h; a.P = side * side;
    a.fxv = r.fxv; a.fyv = r.fyv; a.cxv = r.cxv; a.cyv = r.cyv;
    a.th = r.th;
    Maps m{};
    m.normal_v = Nv; m.dist_v = dist_v;
    Cam cv;
    load_cam(camv, cv);
    float total = 0.f;
    int cnt = 0;
    for (int k = 0; k < r.K; ++k) {
        const MrgsRefScoreNeighbour& nb = nbrs[k];
        Cam cn;
        load_cam(nb.cam, cn);
        a.fxn = (double)nb.fx; a.fyn = (double)nb.fy; a.cxn = (double)nb.cx; a.cyn = (double)nb.cy;
        bool valid = false;
        if (in) {
            const GeoOut g = geo_pixel(a, cv, cn, nb.depth, x, y, dv);
            valid = is_valid(a, g);
        }
        if (__ballot(valid) == 0ull) continue;              // wave-uniform
        if (valid) {
            double Hs[9];
            homography(a, cv, cn, m, p, Hs);
            const float* __restrict__ img_n = nb.image;
            float acc = 0.f;
            for (int oy = 0; oy < side; ++oy) {
                float row = 0.f;
                for (int ox = 0; ox < side; ++ox) {
                    const Foot f = nbr_foot(a, Hs, x + ox - r.h, y + oy - r.h);
                    for (int c = 0; c < 3; ++c) row += fabsf(bil(a, f, img_n + c * HW) - tile[c][ly + oy][lx + ox]);
                }
                acc += row;
            }
            total += acc;
            ++cnt;
        }
    }
    if (in) {
        score[p] = cnt > 0 ? total / ((float)cnt + 1e-8f) / (float)(side * side) : 0.f;
        if (count) count[p] = cnt;
    }
}

}   // namespace

extern "C" int mrgs_ref_score(const MrgsRefScoreConfig* cfg, const float* depth_v, const float* normal_v, const float* distance_v,
                              const float* image_v, const float* cam_v, const MrgsRefScoreNeighbour* neighbours_dev, float* score, int32_t* count,
                              void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsRefScoreConfig)) return MRGS_E_BAD_ARG;
    if (cfg->H <= 0 || cfg->W <= 0 || (int64_t)cfg->H * cfg->W >= ((int64_t)1 << 30)) return MRGS_E_BAD_ARG;
    if (cfg->patch_half < 1 || cfg->patch_half > 4 || cfg->n_neighbours < 0) return MRGS_E_BAD_ARG;
    const float f[5] = {cfg->fx_v, cfg->fy_v, cfg->cx_v, cfg->cy_v, cfg->pixel_noise_th};
    for (int i = 0; i < 5; ++i)
        if (!(f[i] == f[i]) || (i < 2 && !(f[i] > 0.f))) return MRGS_E_BAD_ARG;
    if (!depth_v || !normal_v || !distance_v || !image_v || !cam_v || !score) return MRGS_E_BAD_ARG;
    if (cfg->n_neighbours > 0 && !neighbours_dev) return MRGS_E_BAD_ARG;
    RefArgs r;
    r.H = cfg->H; r.W = cfg->W; r.h = cfg->patch_half; r.K = cfg->n_neighbours;
    r.fxv = cfg->fx_v; r.fyv = cfg->fy_v; r.cxv = cfg->cx_v; r.cyv = cfg->cy_v;
    r.th = cfg->pixel_noise_th;
    const int64_t nblk = (int64_t)((r.W + RS_B - 1) / RS_B) * ((r.H + RS_B - 1) / RS_B);      // < 2^30
    ref_score_fwd<<<(unsigned)nblk, 64, 0, (hipStream_t)stream>>>(r, depth_v, normal_v, distance_v, image_v, cam_v, neighbours_dev, score, count);
    return MRGS_LAUNCH_STATUS();
}
