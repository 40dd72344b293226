// The surfel tracer's hierarchy (mrgs_surfel_trace.hip walks it; mrgs_surfel_trace.h holds the layouts both files share).
// BUILD ON THE DEVICE, every iteration (the reference rebuilds per iteration too, optix_utils.py:68-82): quad boxes + scene bounds (per-block
// partials, folded by the last block: no same-address atomics) -> 30-bit Morton keys -> the radix sort of mrgs_sort.hip -> a complete 64-ARY
// tree over the sorted order, one kernel per level (3-4 levels): node n of level l owns nodes 64 n .. 64 n + 63 of level l-1,
// level 0 owns surfels.  A node is six rows of 64 floats: child c's box is read by LANE c.  ~0.2 ms for 300 k surfels.
// Compiled with -ffp-contract=off like the tracer.
#include <cmath>

#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_surfel_trace.h"

namespace {

constexpr int ST_AABB_BLOCKS = 256;

struct BuildWs {
    size_t aabb, key0, key1, val0, val1, sortws, bounds, total, zero_from, zero_bytes;
};

BuildWs st_build_ws(int64_t P)
{
    BuildWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = mrgs_align_up(o + bytes, 256); return at; };
    w.aabb = take((size_t)P * 24);
    w.key0 = take((size_t)P * 4); w.key1 = take((size_t)P * 4);
    w.val0 = take((size_t)P * 4); w.val1 = take((size_t)P * 4);
    w.zero_from = o;
    w.sortws = take(mrgs_sort_ws_words(P) * 4);
    w.bounds = take(64 + ST_AABB_BLOCKS * 6 * 4);   // 6 ordered-uint extrema, [8] sort error flag, [9] ticket, [16..] per-block partial extrema
    w.zero_bytes = o - w.zero_from;
    w.total = o;
    return w;
}

// quad boxes + scene bounds.  bounds[k] = max ord(hi_k), bounds[3 + k] = max ~ord(lo_k).  Same-address atomics serialise at L2
// (one per wave cost 0.32 ms at 300 k surfels): every block leaves one partial row instead and the last block to finish folds them.
__global__ __launch_bounds__(256) void st_aabb_kernel(int P, const float* __restrict__ verts, float* __restrict__ aabb, uint32_t* __restrict__ partial,
                                                      uint32_t* __restrict__ ticket, uint32_t* __restrict__ bounds)
{
    uint32_t ext[6] = {0, 0, 0, 0, 0, 0};
    for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
        const float4* q = reinterpret_cast<const float4*>(verts + (size_t)p * 12);
        const float4 a = q[0], b = q[1], c = q[2];
        const float v[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            ok = ok && (fabsf(v[i]) < 1e30f);            // false for NaN / inf
            lo[i % 3] = fminf(lo[i % 3], v[i]);
            hi[i % 3] = fmaxf(hi[i % 3], v[i]);
        }
        float* o = aabb + (size_t)p * 6;
        if (ok) {
            o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) { ext[k] = max(ext[k], ord_f(hi[k])); ext[3 + k] = max(ext[3 + k], ~ord_f(lo[k])); }
        } else {
            o[0] = NAN; o[1] = o[2] = o[3] = o[4] = o[5] = 0.f;          // never hit, sorted to key 0
        }
    }
    grid_max6_last_block_folds(ext, partial, ticket, bounds);
}

// Bits of the Morton key per axis.  8: a 24-bit key = THREE 8-bit radix passes instead of four (13 us per traced view); 16.7 M cells for
// leaf groups of 64 surfels is far finer than the groups (measured: the walks take the same time as with 10 bits per axis).
#ifndef ST_MORTON_AXIS_BITS
#define ST_MORTON_AXIS_BITS 8
#endif

__global__ __launch_bounds__(256) void st_morton_kernel(int P, const float* __restrict__ aabb, const uint32_t* __restrict__ bounds,
                                                        uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* b = aabb + (size_t)p * 6;
    uint32_t code = 0;
    if (b[0] == b[0]) {
        uint32_t q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float smin = unord_f(~bounds[3 + k]), smax = unord_f(bounds[k]);
            const float ext = smax - smin;
            const float c = 0.5f * (b[k] + b[3 + k]);
            const float f = ext > 0.f ? (c - smin) / ext : 0.f;
            q[k] = (uint32_t)fminf(fmaxf(f * (float)(1 << ST_MORTON_AXIS_BITS), 0.f), (float)((1 << ST_MORTON_AXIS_BITS) - 1));
        }
        code = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
    }
    key[p] = code;
    val[p] = (uint32_t)p;
}

// One level of the 64-ary tree (64 children per node, stored one child per LANE; why: mrgs_surfel_walk.h).  Level 0 pads the surfels' own
// boxes, every level folds its nodes' boxes into the level above.
// boxes [node][6][64] (lo.xyz, hi.xyz rows), vmask [node]: the children that exist and hold a finite box
__global__ __launch_bounds__(64) void st_wide_level_kernel(int level, int n_children_total, StWide w, const uint32_t* __restrict__ sorted,
                                                           const float* __restrict__ aabb, float* __restrict__ boxes,
                                                           unsigned long long* __restrict__ vmask)
{
    const int node = blockIdx.x, c = threadIdx.x;
    float* mine = boxes + (size_t)(w.off[level] + node) * 384;
    const int child = 64 * node + c;
    bool ok = child < n_children_total;
    float b[6] = {0, 0, 0, 0, 0, 0};
    if (level == 0) {
        if (ok) {
            const float* src = aabb + (size_t)sorted[child] * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) b[k] = src[k];
            ok = b[0] == b[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float pad = 1e-5f * fmaxf(fabsf(b[k]), fabsf(b[3 + k])) + 1e-30f;
                b[k] -= pad; b[3 + k] += pad;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) mine[k * 64 + c] = ok ? b[k] : 0.f;
    } else {
        if (ok) {
#pragma unroll
            for (int k = 0; k < 6; ++k) b[k] = mine[k * 64 + c];       // written by the launch of the level below
            ok = b[0] <= b[3];                                           // a subtree without a valid surfel arrives inverted
        }
    }
    const unsigned long long m = __ballot(ok);
    if (c == 0) vmask[w.off[level] + node] = m;
    if (level + 1 < w.n) {
        float* up = boxes + (size_t)(w.off[level + 1] + (node >> 6)) * 384;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float lo = wave_dpp_min(ok ? b[k] : INFINITY), hi = wave_dpp_max(ok ? b[3 + k] : -INFINITY);
            if (c == 0) { up[k * 64 + (node & 63)] = lo; up[(3 + k) * 64 + (node & 63)] = hi; }
        }
    }
}

}   // namespace

extern "C" {

size_t mrgs_surfel_bvh_bytes(int64_t n_surfels)
{
    if (n_surfels < 0) return 0;
    return st_blob(n_surfels).total;
}

size_t mrgs_surfel_bvh_ws_bytes(int64_t n_surfels)
{
    if (n_surfels < 0) return 0;
    return st_build_ws(n_surfels).total;
}

int mrgs_surfel_bvh_build(const float* quad_vertices, int64_t n_surfels, void* blob, size_t blob_bytes, void* ws, size_t ws_bytes, void* stream)
{
    if (n_surfels < 0 || n_surfels > (int64_t)1 << 24) return MRGS_E_UNSUPPORTED;      // 64^4 surfels
    if (n_surfels == 0) return MRGS_OK;
    if (!quad_vertices || !blob || !ws) return MRGS_E_BAD_ARG;
    const BuildWs w = st_build_ws(n_surfels);
    if (blob_bytes < mrgs_surfel_bvh_bytes(n_surfels) || ws_bytes < w.total) return MRGS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    const int P = (int)n_surfels;
    MRGS_HIP_TRY(hipMemsetAsync(base + w.zero_from, 0, w.zero_bytes, st));
    float* aabb = (float*)(base + w.aabb);
    uint32_t* bounds = (uint32_t*)(base + w.bounds);
    uint32_t* key[2] = {(uint32_t*)(base + w.key0), (uint32_t*)(base + w.key1)};
    uint32_t* val[2] = {(uint32_t*)(base + w.val0), (uint32_t*)(base + w.val1)};
    const int nb = (P + 255) / 256;
    hipLaunchKernelGGL(st_aabb_kernel, dim3(nb < ST_AABB_BLOCKS ? nb : ST_AABB_BLOCKS), dim3(256), 0, st, P, quad_vertices, aabb, bounds + 16,
                       bounds + 9, bounds);
    hipLaunchKernelGGL(st_morton_kernel, dim3(nb), dim3(256), 0, st, P, aabb, bounds, key[0], val[0]);
    const int cur = mrgs_radix_sort_pairs(key, val, (uint32_t*)(base + w.sortws), bounds + 8, n_surfels, nullptr, 0, 3 * ST_MORTON_AXIS_BITS <= 24 ? 24 : 32, st);
    MRGS_HIP_TRY(hipMemcpyAsync(blob, val[cur], (size_t)P * 4, hipMemcpyDeviceToDevice, st));      // the sorted order
    const StWide wd = st_wide(n_surfels);
    const BlobLayout bl = st_blob(n_surfels);
    for (int l = 0; l < wd.n; ++l)
        hipLaunchKernelGGL(st_wide_level_kernel, dim3(wd.cnt[l]), dim3(64), 0, st, l, l == 0 ? P : wd.cnt[l - 1], wd, val[cur], aabb,
                           (float*)((char*)blob + bl.wide_boxes), (unsigned long long*)((char*)blob + bl.wide_vmask));
    return MRGS_LAUNCH_STATUS();
}

}   // extern "C"
