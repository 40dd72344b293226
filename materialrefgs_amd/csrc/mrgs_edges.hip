// The edge mask of the multi-view loss: Canny (L1 gradient, 3 x 3 Sobel, hysteresis) and a box dilation of the 8-bit image of the rendered
// normal map, which the reference computes on the host with cv2 (dilated_edges_imgs, utils/image_utils.py:109-116; called at
// train_refnerf.py:447).  The definition is this library's own and is stated in include/mrgs.h, in integers after one fp32 multiply;
// tests/edges_statement.py restates it in numpy.
//
// Four launches, no host read, no allocation, no spin-wait:
//   classify  one workgroup per EDGE_TILE^2 pixels: the tile and a 2-pixel halo of img are read once, quantised and reduced to grey in
//             LDS; Sobel (dx, dy packed in one word) for the tile and a 1-pixel halo in LDS; non-maximum suppression for the tile; then
//             the components INSIDE the tile by the lock-free union-find of mrgs_cc.h on an LDS array.  Writes the class byte (0 none,
//             1 candidate, 2 strong), parent[i] = the smallest pixel of i's component in the tile, and flag[i] = 0.
//   link      one workgroup per tile, a thread per pixel of its first row, first column and last column: the candidate pairs that cross
//             a tile border (of W, NW, N and NE, which cover every 8-connected pair once) are united in the global parent array.  A link
//             always points to a smaller index, so the root of a component is its smallest pixel whatever order the atomics land in.
//   flag      one thread per pixel: a candidate finds its root and stores it over its own link (roots stay roots in this launch, so every
//             walk stays valid); a strong one also sets flag[root] (every writer stores the same 1).
//   dilate    one workgroup per EDGE_TILE^2 outputs: edge = candidate && flag[parent] for the tile and its dilate_size - 1 halo into LDS,
//             the row OR, then the column OR; invert is applied in the store.
// Algorithmic bytes per pixel: 12 read by classify, 6 written; flag and dilate read the class bytes and touch parent only at candidates.
// Measured (dilate_size 7, 12 % candidates): every candidate uniting with its four neighbours in the global array
// took 63.9 us at 800^2 and 120.2 us at 1600^2, the link launch more than half of it; with the unions a candidate N makes redundant
// left out 51 us and 107 us; with the tile-local unions in LDS and a per-pixel border link 47 us and 83 us -- the form kept; with the
// link launch cut to the border pixels and to the rule's unions 45.4 us and 80.1 us (classify 18.5, link 11.5, dilate 10.6, flag 5.6 us
// at 800^2: the link is bound by the latency of its dependent find / CAS chains, not by its thread count).
#include "mrgs_internal.h"
#include "mrgs_cc.h"

namespace {

constexpr int EDGE_TILE = 32;                   // width and height of the classify and the dilate tile
constexpr int EDGE_MAX_DILATE = 31;
constexpr int GREY_W = EDGE_TILE + 4;           // the tile and 2 pixels around it
constexpr int SOBEL_W = EDGE_TILE + 2;          // the tile and 1 pixel around it
constexpr int DIL_W = EDGE_TILE + EDGE_MAX_DILATE - 1;

struct EdgeArgs {
    int H, W, tiles_x;
    int low, high;                              // floor of the smaller / larger threshold, clamped to [-1, 2041] (m lies in [0, 2040])
    int dilate, invert;
};

// step 1 of the definition
__device__ __forceinline__ int edge_quantise(float x)
{
    const float v = x * 255.0f;
    if (!(fabsf(v) < 2147483648.0f)) return 0;  // NaN, infinities and what does not fit an int32
    return (int)v & 255;
}

__device__ __forceinline__ int sobel_dx(int w) { return (int)(short)(w & 0xFFFF); }
__device__ __forceinline__ int sobel_dy(int w) { return w >> 16; }
__device__ __forceinline__ int sobel_m(int w) { return abs(sobel_dx(w)) + abs(sobel_dy(w)); }

__global__ __launch_bounds__(256) void edge_classify_kernel(EdgeArgs a, const float* __restrict__ img, uint8_t* __restrict__ cls,
                                                            int* __restrict__ parent, uint8_t* __restrict__ flag)
{
    __shared__ int s_grey[GREY_W * GREY_W];
    __shared__ int s_sobel[SOBEL_W * SOBEL_W];
    __shared__ int s_par[EDGE_TILE * EDGE_TILE];
    __shared__ uint8_t s_cls[EDGE_TILE * EDGE_TILE];
    const int x0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * EDGE_TILE, y0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * EDGE_TILE;
    const size_t plane = (size_t)a.H * a.W;
    for (int t = threadIdx.x; t < GREY_W * GREY_W; t += 256) {
        const int ly = t / GREY_W, lx = t - ly * GREY_W;
        const int y = min(max(y0 + ly - 2, 0), a.H - 1), x = min(max(x0 + lx - 2, 0), a.W - 1);     // replicate border
        const size_t i = (size_t)y * a.W + x;
        const int r = edge_quantise(img[i]), g = edge_quantise(img[plane + i]), b = edge_quantise(img[2 * plane + i]);
        s_grey[t] = (9798 * r + 19235 * g + 3735 * b + 16384) >> 15;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < SOBEL_W * SOBEL_W; t += 256) {
        const int ly = t / SOBEL_W, lx = t - ly * SOBEL_W;
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        int w = 0;                                                      // m = 0 outside the image
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const int* g = s_grey + (ly + 1) * GREY_W + (lx + 1);       // this pixel in the grey tile
            const int dx = (g[-GREY_W + 1] + 2 * g[1] + g[GREY_W + 1]) - (g[-GREY_W - 1] + 2 * g[-1] + g[GREY_W - 1]);
            const int dy = (g[GREY_W - 1] + 2 * g[GREY_W] + g[GREY_W + 1]) - (g[-GREY_W - 1] + 2 * g[-GREY_W] + g[-GREY_W + 1]);
            w = (int)((unsigned)(dx & 0xFFFF) | ((unsigned)dy << 16));
        }
        s_sobel[t] = w;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < EDGE_TILE * EDGE_TILE; t += 256) {
        const int ly = t / EDGE_TILE, lx = t - ly * EDGE_TILE;
        int c = 0;
        if (y0 + ly < a.H && x0 + lx < a.W) {
            const int* s = s_sobel + (ly + 1) * SOBEL_W + (lx + 1);
            const int w = s[0], dx = sobel_dx(w), dy = sobel_dy(w), m = abs(dx) + abs(dy);
            if (m > a.low) {
                const int ax = abs(dx), ay = abs(dy) << 15, t22 = ax * 13573, t67 = t22 + (ax << 16);
                bool peak;
                if (ay < t22) peak = m > sobel_m(s[-1]) && m >= sobel_m(s[1]);
                else if (ay > t67) peak = m > sobel_m(s[-SOBEL_W]) && m >= sobel_m(s[SOBEL_W]);
                else {
                    const int sg = ((dx ^ dy) < 0) ? -1 : 1;
                    peak = m > sobel_m(s[-SOBEL_W - sg]) && m > sobel_m(s[SOBEL_W + sg]);
                }
                if (peak) c = m > a.high ? 2 : 1;
            }
        }
        s_cls[t] = (uint8_t)c;
        s_par[t] = t;
    }
    __syncthreads();
    // The components inside the tile, in LDS.  W, NW, N and NE cover every 8-connected pair once, and they are one another's neighbours,
    // so fewer unions do: a candidate N is tied to NW and NE by its own row's threads (NW is its W, it is NE's W) and to W by W's thread
    // (N is W's NE, or both hang on NW = W's N): N alone.  Otherwise W, NE, and NW unless W has it (its N).  A neighbour outside the tile
    // counts as absent here, which only adds unions; edge_link_kernel makes the pairs of the rule that leave the tile.
    for (int t = threadIdx.x; t < EDGE_TILE * EDGE_TILE; t += 256) {
        if (!s_cls[t]) continue;
        const int ly = t / EDGE_TILE, lx = t - ly * EDGE_TILE;
        const bool w = lx > 0 && s_cls[t - 1];
        if (ly > 0) {
            const int up = t - EDGE_TILE;
            if (s_cls[up]) { cc_union(s_par, t, up); continue; }
            if (!w && lx > 0 && s_cls[up - 1]) cc_union(s_par, t, up - 1);
            if (lx + 1 < EDGE_TILE && s_cls[up + 1]) cc_union(s_par, t, up + 1);
        }
        if (w) cc_union(s_par, t, t - 1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < EDGE_TILE * EDGE_TILE; t += 256) {
        const int ly = t / EDGE_TILE, lx = t - ly * EDGE_TILE;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= a.H || x >= a.W) continue;
        const int r = cc_find(s_par, t);                                // the smallest index of the component in the tile, local and global
        const size_t i = (size_t)y * a.W + x;
        cls[i] = s_cls[t];
        parent[i] = (y0 + r / EDGE_TILE) * a.W + x0 + r % EDGE_TILE;
        flag[i] = 0;
    }
}

// the pairs that cross a tile border: W of a tile's first column, N of its first row, NW of either, NE of the first row and the last column.
// One workgroup per tile, a thread per pixel of those three sides.
__global__ __launch_bounds__(4 * EDGE_TILE) void edge_link_kernel(EdgeArgs a, const uint8_t* __restrict__ cls, int* parent)
{
    const int x0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * EDGE_TILE, y0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * EDGE_TILE;
    const int k = threadIdx.x % EDGE_TILE, side = threadIdx.x / EDGE_TILE;           // 0 first row, 1 first column, 2 last column
    if (side > 2 || (side > 0 && k == 0)) return;                                   // the corners belong to the row
    const int ly = side == 0 ? 0 : k, lx = side == 0 ? k : side == 1 ? 0 : EDGE_TILE - 1;
    const int y = y0 + ly, x = x0 + lx, W = a.W;
    if (y >= a.H || x >= W) return;
    const long long i = (long long)y * W + x;
    if (!cls[i]) return;
    // the rule of the tile-local unions with the true neighbours; of its pairs, those that leave the tile
    const bool top = ly == 0, left = lx == 0, right = lx == EDGE_TILE - 1;
    const long long up = i - W;
    if (y > 0 && cls[up]) {
        if (top) cc_union(parent, (int)i, (int)up);
        return;
    }
    const bool w = x > 0 && cls[i - 1];
    if (y > 0) {
        if ((top || left) && !w && x > 0 && cls[up - 1]) cc_union(parent, (int)i, (int)up - 1);
        if ((top || right) && x + 1 < W && cls[up + 1]) cc_union(parent, (int)i, (int)up + 1);
    }
    if (left && w) cc_union(parent, (int)i, (int)i - 1);
}

__global__ __launch_bounds__(256) void edge_flag_kernel(long long n, const uint8_t* __restrict__ cls, int* parent, uint8_t* flag)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cls[i];
    if (!c) return;
    const int r = cc_find(parent, (int)i);
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c == 2) flag[r] = 1;
}

__global__ __launch_bounds__(256) void edge_dilate_kernel(EdgeArgs a, const uint8_t* __restrict__ cls, const int* __restrict__ parent,
                                                          const uint8_t* __restrict__ flag, uint8_t* __restrict__ out)
{
    __shared__ uint8_t s_edge[DIL_W * DIL_W];
    __shared__ uint8_t s_row[DIL_W * EDGE_TILE];
    const int x0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * EDGE_TILE, y0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * EDGE_TILE;
    const int d = a.dilate, anchor = d / 2, ext = EDGE_TILE + d - 1;    // the window of an output is [-anchor, d - 1 - anchor] both ways
    for (int t = threadIdx.x; t < ext * ext; t += 256) {
        const int ly = t / ext, lx = t - ly * ext;
        const int y = y0 + ly - anchor, x = x0 + lx - anchor;
        uint8_t e = 0;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const size_t i = (size_t)y * a.W + x;
            if (cls[i]) e = flag[parent[i]];                            // parent[i] is the root since the flag launch
        }
        s_edge[ly * DIL_W + lx] = e;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ext * EDGE_TILE; t += 256) {
        const int ly = t / EDGE_TILE, lx = t - ly * EDGE_TILE;
        uint8_t e = 0;
        for (int k = 0; k < d; ++k) e |= s_edge[ly * DIL_W + lx + k];
        s_row[t] = e;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < EDGE_TILE * EDGE_TILE; t += 256) {
        const int ly = t / EDGE_TILE, lx = t - ly * EDGE_TILE;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= a.H || x >= a.W) continue;
        uint8_t e = 0;
        for (int k = 0; k < d; ++k) e |= s_row[(ly + k) * EDGE_TILE + lx];
        out[(size_t)y * a.W + x] = (uint8_t)((e ? 1 : 0) ^ a.invert);
    }
}

struct EdgeWs { int* parent; uint8_t* cls; uint8_t* flag; size_t total; };

EdgeWs edge_carve(void* base, size_t n)
{
    const size_t cls = mrgs_align_up(n * sizeof(int), 256), flag = cls + mrgs_align_up(n, 256);
    EdgeWs w = {};
    w.total = flag + mrgs_align_up(n, 256);
    if (base) {                                                         // the size query carves nothing
        uint8_t* p = (uint8_t*)base;
        w.parent = (int*)p; w.cls = p + cls; w.flag = p + flag;
    }
    return w;
}

int edge_threshold(float t)
{
    const float f = floorf(t);
    return f < -1.0f ? -1 : f > 2041.0f ? 2041 : (int)f;
}

}   // namespace

extern "C" size_t mrgs_edges_ws_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return 0;
    return edge_carve(nullptr, (size_t)H * W).total;
}

extern "C" int mrgs_edge_mask(const float* img, int32_t H, int32_t W, int32_t dilate_size, float thres1, float thres2, int32_t invert,
                              uint8_t* out, uint8_t* classes_out, void* ws, size_t ws_bytes, void* stream)
{
    if (H <= 0 || W <= 0 || dilate_size < 1 || dilate_size > EDGE_MAX_DILATE || !(thres1 == thres1) || !(thres2 == thres2)) return MRGS_E_BAD_ARG;
    if (!img || !out || !ws || ((uintptr_t)ws & 3)) return MRGS_E_BAD_ARG;
    const long long n = (long long)H * W;
    if (n >= (1ll << 31)) return MRGS_E_UNSUPPORTED;
    if (ws_bytes < mrgs_edges_ws_bytes(H, W)) return MRGS_E_WORKSPACE;
    const EdgeWs w = edge_carve(ws, (size_t)n);
    uint8_t* cls = classes_out ? classes_out : w.cls;
    EdgeArgs a;
    a.H = H; a.W = W; a.tiles_x = (W + EDGE_TILE - 1) / EDGE_TILE;
    a.low = edge_threshold(thres1 < thres2 ? thres1 : thres2);
    a.high = edge_threshold(thres1 < thres2 ? thres2 : thres1);
    a.dilate = dilate_size; a.invert = invert ? 1 : 0;
    const long long tiles = (long long)a.tiles_x * ((H + EDGE_TILE - 1) / EDGE_TILE);       // < 2^31: at most ~2^31 / 32 + 1 tiles of a 1 x W image
    const dim3 tile_grid((unsigned)tiles), pixel_grid((unsigned)((n + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    edge_classify_kernel<<<tile_grid, 256, 0, st>>>(a, img, cls, w.parent, w.flag);
    edge_link_kernel<<<tile_grid, 4 * EDGE_TILE, 0, st>>>(a, cls, w.parent);
    edge_flag_kernel<<<pixel_grid, 256, 0, st>>>(n, cls, w.parent, w.flag);
    edge_dilate_kernel<<<tile_grid, 256, 0, st>>>(a, cls, w.parent, w.flag, out);
    return MRGS_LAUNCH_STATUS();
}
