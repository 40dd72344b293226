// The Sobel smoothness terms of one view, fused: smooth_loss (utils/loss_utils.py:124-125; train_refreal.py:1261 adds it on the masked base
// colour) and first_order_edge_aware_loss (:121-122; calculate_loss :185-197 adds it on rend_normal and surf_depth).  In torch a pad, a
// reshape and a conv2d per operand, abs / exp / mul / sum / mean and the same chain again in backward with a transposed convolution: some
// twenty launches a term.  Here up to SMOOTH_MAX_ITEMS maps over the same H x W in
//   smooth_terms_fwd        one workgroup per SMOOTH_TILE^2 pixels, a bounded grid that strides over the tiles: a plane of the tile and a
//                           1-pixel halo (replicate border: clamped coordinates; all of a thread's loads before its first LDS store; an
//                           item's mask read once per tile) goes to LDS, each thread takes the Sobel pair of its four pixels from it.  The image's weights exp(-|G(img_c)|) are formed once per tile into LDS and serve every edge-aware
//                           item.  A thread sums its pixels over all of its tiles, then the wave, then the four waves in a fixed order into
//                           one row per workgroup;
//   smooth_terms_finalize   one workgroup sums the rows in double in a fixed order and divides by the item's element count;
//   smooth_terms_bwd        one launch, a gather: S_dir(p) = sign(G_dir(p)) w_dir(p) for the tile and a 1-pixel halo (0 outside the image) from
//                           a plane with a 2-pixel halo; an output texel q sums coefficient x S over the source pixels whose clamped taps
//                           land on it.
// No atomics: both directions are run-to-run identical.  No host read.
//
// Definitions.  G_x(p) = sum_{dy,dx} s(dy) d(dx) x(clamp(p + (dy, dx))) / 8 with s = (1, 2, 1), d = (-1, 0, 1) over the offsets (-1, 0, 1),
// G_y the same with the roles of the axes swapped: losses.spatial_gradient.  d|G|/dG = sign(G), sign(0) = 0.
// The adjoint of the clamped stencil.  The clamp acts per axis and the kernel is separable, so
//   dL/dx(q) = 1/8 sum_p [ A(q_y, p_y; H) B(q_x, p_x; W) S_x(p) + B(q_y, p_y; H) A(q_x, p_x; W) S_y(p) ],
//   A(q, p; n) = sum_e s(e) [clamp(p + e, 0, n - 1) = q],  B(q, p; n) = sum_e d(e) [clamp(p + e, 0, n - 1) = q],
// over the source pixels p of the image; both vanish unless |p - q| <= 1 (a tap that leaves the image comes back to the border, never
// further in).  For an inner q these are (1, 2, 1) and (1, 0, -1); at a border the taps of the padded ring fold into them (A(0, 0) = 3,
// B(0, 0) = -1; a corner folds three ring positions), and when n is 1 or 2 one texel is first and last at once and takes the folds of
// both sides (n = 1: A(0, 0) = 4, B(0, 0) = 0).  fold_weights below evaluates the definition as it stands.
#include "mrgs_internal.h"
#include "mrgs_wave.h"

namespace {

constexpr int SMOOTH_TILE = 32;               // width and height of a tile
constexpr int SMOOTH_MAX_BLOCKS = 1024;       // four workgroups per CU
constexpr int PX = SMOOTH_TILE * SMOOTH_TILE / 256;      // pixels of a tile per thread: rows ly = (tid >> 5) + 8 k of column tid & 31
constexpr int FWD_W = SMOOTH_TILE + 2;        // forward: the plane with a 1-pixel halo
constexpr int BWD_IN_W = SMOOTH_TILE + 4;     // backward: the plane with a 2-pixel halo ...
constexpr int BWD_S_W = SMOOTH_TILE + 2;      // ... gives S on the tile and a 1-pixel halo
static_assert(MRGS_SMOOTH_MAX_ITEMS == 4, "a row of partial sums is one 16-byte word");

struct SmoothItem {
    const float* data;           // [C,H,W]
    const uint8_t* mask;         // [H W] or null
    float* g_data;               // backward: [C,H,W] or null
    const float* g;              // backward: the upstream gradient, a device scalar, null = 0
    int C, edge;
};

struct SmoothArgs {
    int H, W, tiles_x, n_items;
    long long tiles;
    const float* img;            // [3,H,W]; null when no item is edge-aware
    int any_edge;                // some item the launch works on is edge-aware
    SmoothItem items[MRGS_SMOOTH_MAX_ITEMS];
};

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// The staging of a tile at (y0, x0) with R pixels around it: thread tid takes the texels tid + 256 k of the (SMOOTH_TILE + 2 R)^2 region, the
// same ones for every plane, so an item's mask is read once per tile and kept as one bit per texel.
template <int R>
struct Stage {
    static constexpr int IN_W = SMOOTH_TILE + 2 * R, N = (IN_W * IN_W + 255) / 256;
    // the global index of texel k of this thread: replicate border; the last round's spare threads take the last texel again
    static __device__ __forceinline__ size_t index(int k, int y0, int x0, int H, int W)
    {
        const int t = min((int)threadIdx.x + 256 * k, IN_W * IN_W - 1);
        const int ly = t / IN_W, lx = t - ly * IN_W;
        const int y = min(max(y0 + ly - R, 0), H - 1), x = min(max(x0 + lx - R, 0), W - 1);
        return (size_t)y * W + x;
    }
    // bit k: texel k is kept (all of them without a mask)
    static __device__ __forceinline__ uint32_t mask_bits(const uint8_t* __restrict__ mask, int y0, int x0, int H, int W)
    {
        if (!mask) return ~0u;
        uint8_t m[N];
#pragma unroll
        for (int k = 0; k < N; ++k) m[k] = mask[index(k, y0, x0, H, W)];
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) bits |= (m[k] ? 1u : 0u) << k;
        return bits;
    }
    // a plane into LDS, the mask applied before the stencil.  Every load of the thread is issued before the first one is waited for: with
    // the load and the LDS store in one loop body the N round trips to memory ran one behind the other
    static __device__ __forceinline__ void plane(float* __restrict__ s, const float* __restrict__ src, uint32_t keep, int y0, int x0, int H, int W)
    {
        float v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = src[index(k, y0, x0, H, W)];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int t = threadIdx.x + 256 * k;
            if (t < IN_W * IN_W) s[t] = (keep >> k) & 1u ? v[k] : 0.f;
        }
    }
};

// bit k: the thread's own pixel k of the tile (row ly0 + 8 k, column lx) is kept; pixels outside the image count as kept, nothing is written there
__device__ __forceinline__ uint32_t own_mask_bits(const uint8_t* __restrict__ mask, int y0, int x0, int ly0, int lx, int H, int W)
{
    if (!mask) return ~0u;
    uint8_t m[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) m[k] = mask[(size_t)min(y0 + ly0 + 8 * k, H - 1) * W + min(x0 + lx, W - 1)];
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < PX; ++k) bits |= (m[k] ? 1u : 0u) << k;
    return bits;
}

// 8 G_x and 8 G_y at the centre s of a staged plane with row stride st
__device__ __forceinline__ void sobel8(const float* __restrict__ s, int st, float& gx, float& gy)
{
    const float nw = s[-st - 1], n = s[-st], ne = s[-st + 1], w = s[-1], e = s[1], sw = s[st - 1], so = s[st], se = s[st + 1];
    gx = (ne + 2.f * e + se) - (nw + 2.f * w + sw);
    gy = (sw + 2.f * so + se) - (nw + 2.f * n + ne);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smooth_terms_fwd(SmoothArgs a, float* __restrict__ partials)
{
    __shared__ float s_in[FWD_W * FWD_W];
    __shared__ float s_w[6][SMOOTH_TILE * SMOOTH_TILE];           // exp(-|G_x|), exp(-|G_y|) of the image's three channels
    __shared__ float red[4][MRGS_SMOOTH_MAX_ITEMS];
    const int tid = threadIdx.x, lx = tid & (SMOOTH_TILE - 1), ly0 = tid / SMOOTH_TILE;
    const size_t plane = (size_t)a.H * a.W;
    float acc[MRGS_SMOOTH_MAX_ITEMS] = {0.f, 0.f, 0.f, 0.f};
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int y0 = (int)(tile / a.tiles_x) * SMOOTH_TILE, x0 = (int)(tile % a.tiles_x) * SMOOTH_TILE;
        if (a.any_edge) {
            for (int c = 0; c < 3; ++c) {
                Stage<1>::plane(s_in, a.img + c * plane, ~0u, y0, x0, a.H, a.W);
                __syncthreads();
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int ly = ly0 + 8 * k;
                    float gx, gy;
                    sobel8(s_in + (ly + 1) * FWD_W + lx + 1, FWD_W, gx, gy);
                    s_w[2 * c][ly * SMOOTH_TILE + lx] = expf(-0.125f * fabsf(gx));
                    s_w[2 * c + 1][ly * SMOOTH_TILE + lx] = expf(-0.125f * fabsf(gy));
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int i = 0; i < MRGS_SMOOTH_MAX_ITEMS; ++i) {          // unrolled: the items and the sums are indexed by constants
            if (i >= a.n_items) break;
            const SmoothItem& it = a.items[i];
            const uint32_t keep = Stage<1>::mask_bits(it.mask, y0, x0, a.H, a.W);
            for (int c = 0; c < it.C; ++c) {
                Stage<1>::plane(s_in, it.data + c * plane, keep, y0, x0, a.H, a.W);
                __syncthreads();
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int ly = ly0 + 8 * k, t = ly * SMOOTH_TILE + lx;
                    if (y0 + ly < a.H && x0 + lx < a.W) {
                        float gx, gy;
                        sobel8(s_in + (ly + 1) * FWD_W + lx + 1, FWD_W, gx, gy);
                        float wx = 1.f, wy = 1.f;
                        if (it.edge) {                            // C = 1: the one map against each of the image's channels
                            wx = it.C == 3 ? s_w[2 * c][t] : (s_w[0][t] + s_w[2][t]) + s_w[4][t];
                            wy = it.C == 3 ? s_w[2 * c + 1][t] : (s_w[1][t] + s_w[3][t]) + s_w[5][t];
                        }
                        acc[i] += fabsf(gx) * wx + fabsf(gy) * wy;
                    }
                }
                __syncthreads();
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MRGS_SMOOTH_MAX_ITEMS; ++i) {
        const float v = wave_shfl_sum(acc[i]);
        if ((tid & 63) == 0) red[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid < MRGS_SMOOTH_MAX_ITEMS) partials[(size_t)blockIdx.x * MRGS_SMOOTH_MAX_ITEMS + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// the element count of an item's mean: C H W of a plain item, 3 H W of an edge-aware one (C = 1 broadcasts against the image's channels)
__host__ __device__ __forceinline__ double smooth_count(int C, int edge, int H, int W) { return (double)(edge ? 3 : C) * (double)H * (double)W; }

__global__ __launch_bounds__(256) void smooth_terms_finalize(SmoothArgs a, const float* __restrict__ partials, int nblocks, float* __restrict__ out)
{
    __shared__ double red[4][MRGS_SMOOTH_MAX_ITEMS];
    const int tid = threadIdx.x;
    block_rows_sum_256<MRGS_SMOOTH_MAX_ITEMS, MRGS_SMOOTH_MAX_ITEMS>(partials, nblocks, red);
    if (tid < a.n_items) out[tid] = (float)(0.125 * rows_total(red, tid) / smooth_count(a.items[tid].C, a.items[tid].edge, a.H, a.W));
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
// A(q, q + j; n) and B(q, q + j; n) for j = -1, 0, 1 (file header); 0 for a source outside [0, n)
__device__ __forceinline__ void fold_weights(int q, int n, float (&A)[3], float (&B)[3])
{
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int p = q + j;
        float sa = 0.f, sb = 0.f;
        if (p >= 0 && p < n) {
#pragma unroll
            for (int e = -1; e <= 1; ++e) {
                if (min(max(p + e, 0), n - 1) == q) { sa += e == 0 ? 2.f : 1.f; sb += (float)e; }
            }
        }
        A[j + 1] = sa; B[j + 1] = sb;
    }
}

__global__ __launch_bounds__(256) void smooth_terms_bwd(SmoothArgs a)
{
    __shared__ float s_in[BWD_IN_W * BWD_IN_W];
    __shared__ float s_w[6][BWD_S_W * BWD_S_W];
    __shared__ float s_s[2][BWD_S_W * BWD_S_W];
    const int tid = threadIdx.x, lx = tid & (SMOOTH_TILE - 1), ly0 = tid / SMOOTH_TILE;
    const size_t plane = (size_t)a.H * a.W;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int y0 = (int)(tile / a.tiles_x) * SMOOTH_TILE, x0 = (int)(tile % a.tiles_x) * SMOOTH_TILE;
        if (a.any_edge) {
            for (int c = 0; c < 3; ++c) {
                Stage<2>::plane(s_in, a.img + c * plane, ~0u, y0, x0, a.H, a.W);
                __syncthreads();
                for (int t = tid; t < BWD_S_W * BWD_S_W; t += 256) {
                    const int sy = t / BWD_S_W, sx = t - sy * BWD_S_W;
                    float gx, gy;
                    sobel8(s_in + (sy + 1) * BWD_IN_W + sx + 1, BWD_IN_W, gx, gy);
                    s_w[2 * c][t] = expf(-0.125f * fabsf(gx));
                    s_w[2 * c + 1][t] = expf(-0.125f * fabsf(gy));
                }
                __syncthreads();
            }
        }
        // the fold weights of this thread's column and of its PX rows, once per tile: they serve every item and channel
        float Ax[3], Bx[3], Ay[PX][3], By[PX][3];
        fold_weights(x0 + lx, a.W, Ax, Bx);
#pragma unroll
        for (int k = 0; k < PX; ++k) fold_weights(y0 + ly0 + 8 * k, a.H, Ay[k], By[k]);
#pragma unroll
        for (int i = 0; i < MRGS_SMOOTH_MAX_ITEMS; ++i) {
            if (i >= a.n_items) break;
            const SmoothItem& it = a.items[i];
            if (!it.g_data) continue;
            if (!it.g) {                                          // no upstream gradient: the map is zeros, nothing is read
                for (int c = 0; c < it.C; ++c)
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int y = y0 + ly0 + 8 * k, x = x0 + lx;
                        if (y < a.H && x < a.W) it.g_data[c * plane + (size_t)y * a.W + x] = 0.f;
                    }
                continue;
            }
            const float scale = it.g[0] * (float)(0.125 / smooth_count(it.C, it.edge, a.H, a.W));
            const uint32_t keep = Stage<2>::mask_bits(it.mask, y0, x0, a.H, a.W), own = own_mask_bits(it.mask, y0, x0, ly0, lx, a.H, a.W);
            for (int c = 0; c < it.C; ++c) {
                Stage<2>::plane(s_in, it.data + c * plane, keep, y0, x0, a.H, a.W);
                __syncthreads();
                for (int t = tid; t < BWD_S_W * BWD_S_W; t += 256) {
                    const int sy = t / BWD_S_W, sx = t - sy * BWD_S_W;
                    const int y = y0 + sy - 1, x = x0 + sx - 1;
                    float vx = 0.f, vy = 0.f;                     // a source pixel outside the image does not exist
                    if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
                        float gx, gy;
                        sobel8(s_in + (sy + 1) * BWD_IN_W + sx + 1, BWD_IN_W, gx, gy);
                        vx = sgn(gx); vy = sgn(gy);
                        if (it.edge) {
                            vx *= it.C == 3 ? s_w[2 * c][t] : (s_w[0][t] + s_w[2][t]) + s_w[4][t];
                            vy *= it.C == 3 ? s_w[2 * c + 1][t] : (s_w[1][t] + s_w[3][t]) + s_w[5][t];
                        }
                    }
                    s_s[0][t] = vx; s_s[1][t] = vy;
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int ly = ly0 + 8 * k, y = y0 + ly, x = x0 + lx;
                    if (y >= a.H || x >= a.W) continue;
                    float sum = 0.f;
#pragma unroll
                    for (int jy = 0; jy < 3; ++jy) {                            // row by row: the source pixels q + (jy - 1, -1 .. 1)
                        const float* sx = s_s[0] + (ly + jy) * BWD_S_W + lx;
                        const float* sy = s_s[1] + (ly + jy) * BWD_S_W + lx;
                        sum += Ay[k][jy] * ((Bx[0] * sx[0] + Bx[1] * sx[1]) + Bx[2] * sx[2]) + By[k][jy] * ((Ax[0] * sy[0] + Ax[1] * sy[1]) + Ax[2] * sy[2]);
                    }
                    const size_t q = (size_t)y * a.W + x;
                    it.g_data[c * plane + q] = (own >> k) & 1u ? scale * sum : 0.f;      // the gradient passes where the mask is nonzero
                }
                // the next plane's staging writes s_in, which nobody reads any more; s_s is written again only behind the next barrier
            }
        }
    }
}

int smooth_blocks(long long tiles) { return (int)(tiles > SMOOTH_MAX_BLOCKS ? SMOOTH_MAX_BLOCKS : tiles); }
long long smooth_tiles(int H, int W) { return (long long)((H + SMOOTH_TILE - 1) / SMOOTH_TILE) * ((W + SMOOTH_TILE - 1) / SMOOTH_TILE); }

// the checks both directions share
int make_args(const MrgsSmoothConfig* cfg, const float* img, const MrgsSmoothItem* items, int32_t n_items, SmoothArgs& a)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsSmoothConfig) || cfg->H <= 0 || cfg->W <= 0 || cfg->flags != 0) return MRGS_E_BAD_ARG;
    if (!items || n_items < 1 || n_items > MRGS_SMOOTH_MAX_ITEMS) return MRGS_E_BAD_ARG;
    a = SmoothArgs{};
    a.H = cfg->H; a.W = cfg->W; a.tiles_x = (cfg->W + SMOOTH_TILE - 1) / SMOOTH_TILE; a.tiles = smooth_tiles(cfg->H, cfg->W);
    a.n_items = n_items; a.img = img;
    for (int i = 0; i < n_items; ++i) {
        const MrgsSmoothItem& it = items[i];
        if (!it.data || (it.edge_aware != 0 && it.edge_aware != 1)) return MRGS_E_BAD_ARG;
        if (it.edge_aware ? (it.C != 1 && it.C != 3) || !img : (it.C < 1 || it.C > 4)) return MRGS_E_BAD_ARG;
        a.items[i] = {it.data, it.mask, it.g_data, nullptr, it.C, it.edge_aware};
    }
    return MRGS_OK;
}

}   // namespace

extern "C" size_t mrgs_smooth_ws_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return 0;
    return (size_t)smooth_blocks(smooth_tiles(H, W)) * MRGS_SMOOTH_MAX_ITEMS * sizeof(float);
}

extern "C" int mrgs_smooth_terms_forward(const MrgsSmoothConfig* cfg, const float* img, const MrgsSmoothItem* items, int32_t n_items, void* ws,
                                         size_t ws_bytes, float* out_terms, void* stream)
{
    SmoothArgs a;
    if (int rc = make_args(cfg, img, items, n_items, a)) return rc;
    if (!ws || !out_terms || ((uintptr_t)ws & 15) || ws_bytes < mrgs_smooth_ws_bytes(cfg->H, cfg->W)) return MRGS_E_BAD_ARG;
    for (int i = 0; i < n_items; ++i) a.any_edge |= a.items[i].edge;
    const int nblocks = smooth_blocks(a.tiles);
    hipStream_t st = (hipStream_t)stream;
    smooth_terms_fwd<<<nblocks, 256, 0, st>>>(a, (float*)ws);
    smooth_terms_finalize<<<1, 256, 0, st>>>(a, (const float*)ws, nblocks, out_terms);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_smooth_terms_backward(const MrgsSmoothConfig* cfg, const float* img, const MrgsSmoothItem* items, int32_t n_items,
                                          const float* const* g_terms, void* stream)
{
    SmoothArgs a;
    if (int rc = make_args(cfg, img, items, n_items, a)) return rc;
    if (!g_terms) return MRGS_E_BAD_ARG;
    bool any = false;
    for (int i = 0; i < n_items; ++i) {
        if (g_terms[i] && !a.items[i].g_data) return MRGS_E_BAD_ARG;
        a.items[i].g = g_terms[i];
        any |= a.items[i].g_data != nullptr;
        a.any_edge |= a.items[i].edge && a.items[i].g_data && a.items[i].g;      // the weights are formed only for an item that uses them
    }
    if (!any) return MRGS_OK;                                     // nothing to write
    smooth_terms_bwd<<<smooth_blocks(a.tiles), 256, 0, (hipStream_t)stream>>>(a);
    return MRGS_LAUNCH_STATUS();
}
