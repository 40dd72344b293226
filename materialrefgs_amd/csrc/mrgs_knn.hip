// mrgs_knn.hip -- mean squared distance to the three nearest other points: the initial scales of a point cloud.
//
// Replaces simple_knn's distCUDA2 (submodules/simple-knn/simple_knn.cu:147-221 behind spatial.cu:14-26), which GaussianModel.create_from_pcd
// calls once per run (scene/gaussian_model.py:367, env_gaussian_model.py:147): dist[i] = mean over the three nearest points j != i of
// |p_j - p_i|^2.  The reference is CUB + thrust + cooperative groups and walks, one thread per point, every 1024-point box whose distance
// does not exceed the current third value, fetching points[indices[j]] per candidate.
//
// The value is defined without any search structure, and that definition is what is pinned (tests/knn_statement.py):
//   d(i, j) = (dx dx + dy dy) + dz dz in fp32, un-fused (this file is compiled with -ffp-contract=off), dx = fl(p_i.x - p_j.x), ...
//   dist[i] = ((b0 + b1) + b2) / 3.0f, b0 <= b1 <= b2 the three smallest d(i, j) over j != i (by INDEX: a duplicate at another index is
//   a neighbour at distance 0), a missing neighbour counting as FLT_MAX (simple_knn.cu:150).
// The multiset {b0, b1, b2} does not depend on the visiting order or on how ties are broken, so the result is a pure function of the
// input: bitwise repeatable, invariant under a permutation of the rows, bit-equal to the float32 brute force.  (nvcc contracts by
// default: the reference's own values may differ from these in the last bit.)
//
// Everything below only prunes.  Six steps on the caller's stream (one memset, ten launches, five of them the sort's), no host read, no
// allocation:
//   1. knn_bounds_kernel   extent of the finite coordinates (per-block partial rows, the last block folds them: grid_max6_last_block_folds)
//   2. knn_morton_kernel   30-bit Morton key (10 bits per axis; an axis of zero extent gets code 0, the reference divides by zero there:
//                          simple_knn.cu:56-58), value = row index; the float -> integer conversion is clamped first, a non-finite
//                          coordinate lands in cell 0
//   3. mrgs_radix_sort_pairs over bits 0..30 (four onesweep passes)
//   4. knn_gather_kernel   sorted[i] = (x, y, z, row index as bits) in Morton order -- the search reads 16-byte lane-contiguous rows and
//                          chases no index -- and the box of every LEAF = 64 Morton-consecutive points (one wave's queries and one
//                          wave-wide candidate tile)
//   5. knn_top_kernel      the box of every 64 leaves
//   6. knn_search_kernel   one wave per leaf, one query per lane.  Seed: the own leaf and its two neighbours in Morton order (the
//                          reference's +-3 window and more) fill b0..b2.  Walk: lanes test DIFFERENT boxes (64 top boxes per step, then
//                          the 64 leaves of each surviving top box) against the wave's query box and the wave's largest b2; per
//                          surviving leaf the whole wave tests that leaf's box (wave-uniform values) against each lane's own point and b2
//                          (distBoxPoint, simple_knn.cu:119-129) and skips it when no lane needs it, otherwise loads its 64 candidates
//                          with one coalesced 1 KB read and every lane updates its three values over the same candidates, handed round
//                          with v_readlane: no LDS, no per-lane divergence.
// Pruning is exact in fp32: for a candidate c inside a box, |fl(p - c)| >= fl(gap to the box) per axis (rounding is monotonic), and the
// squares and the two sums are monotonic too when taken in the same order, so box distance <= candidate distance AS COMPUTED.  A box is
// skipped when its distance is >= b2 (the reference uses >): a candidate that only ties the third value cannot change the three values,
// and a cluster of identical points stops after its seed instead of being walked quadratically.
// More than 64 top boxes (P > 2^18) are taken 64 at a time: 16 steps at P = 4 M; no third level.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mrgs_internal.h"
#include "mrgs_wave.h"

namespace {

constexpr int KNN_BOUNDS_BLOCKS = 256;
constexpr int KNN_WAVES = 4;                 // waves (= leaves) per workgroup of the gather and the search

struct KnnWs {
    size_t key0, key1, val0, val1, sorted, leafbox, topbox, sortws, bounds, total, zero_from, zero_bytes;
    int64_t L, T;                            // leaves, top boxes
};

KnnWs knn_ws(int64_t P)
{
    KnnWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = mrgs_align_up(o + bytes, 256); return at; };
    w.L = (P + 63) / 64;
    w.T = (w.L + 63) / 64;
    w.key0 = take((size_t)P * 4); w.key1 = take((size_t)P * 4);
    w.val0 = take((size_t)P * 4); w.val1 = take((size_t)P * 4);
    w.sorted = take((size_t)P * 16);
    w.leafbox = take((size_t)w.L * 32);      // (lo.xyz, -) (hi.xyz, -)
    w.topbox = take((size_t)w.T * 32);
    w.zero_from = o;
    w.sortws = take(mrgs_sort_ws_words(P) * 4);
    w.bounds = take(64 + KNN_BOUNDS_BLOCKS * 6 * 4);   // 6 ordered-uint extrema, [8] sort error flag, [9] ticket, [16..] per-block partial extrema
    w.zero_bytes = o - w.zero_from;
    w.total = o;
    return w;
}

// bounds[k] = max ord(x_k), bounds[3 + k] = max ~ord(x_k) over the finite coordinates (a non-finite one is left out: it is clamped into
// the grid later).  One partial row per block, folded by the last block to finish (grid_max6_last_block_folds, as st_aabb_kernel of mrgs_surfel_hier.hip).
__global__ __launch_bounds__(256) void knn_bounds_kernel(int P, const float* __restrict__ pts, uint32_t* __restrict__ partial,
                                                         uint32_t* __restrict__ ticket, uint32_t* __restrict__ bounds)
{
    uint32_t ext[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
        const float* q = pts + (size_t)p * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = q[k];
            if (fabsf(v) <= FLT_MAX) { ext[k] = max(ext[k], ord_f(v)); ext[3 + k] = max(ext[3 + k], ~ord_f(v)); }
        }
    }
    grid_max6_last_block_folds(ext, partial, ticket, bounds);
}

__global__ __launch_bounds__(256) void knn_morton_kernel(int P, const float* __restrict__ pts, const uint32_t* __restrict__ bounds,
                                                         uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* q = pts + (size_t)p * 3;
    uint32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float smin = unord_f(~bounds[3 + k]), smax = unord_f(bounds[k]);
        const float ext = smax - smin;
        // zero extent (or no finite coordinate at all): code 0; a non-finite coordinate: cell 0
        const float f = (ext > 0.f && fabsf(q[k]) <= FLT_MAX) ? (q[k] - smin) / ext : 0.f;
        c[k] = (uint32_t)fminf(fmaxf(f * 1024.f, 0.f), 1023.f);     // clamped BEFORE the conversion; fmaxf(NaN, 0) = 0
    }
    key[p] = (spread10(c[0]) << 2) | (spread10(c[1]) << 1) | spread10(c[2]);
    val[p] = (uint32_t)p;
}

// one wave per leaf: the leaf's points in Morton order and their box
__global__ __launch_bounds__(64 * KNN_WAVES) void knn_gather_kernel(int P, int L, const float* __restrict__ pts, const uint32_t* __restrict__ order,
                                                                    float4* __restrict__ sorted, float4* __restrict__ leafbox)
{
    const int lane = threadIdx.x & 63;
    const int leaf = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * KNN_WAVES + (threadIdx.x >> 6)));
    if (leaf >= L) return;
    const int i = leaf * 64 + lane;
    const bool valid = i < P;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (valid) {
        // (the sort leaves a permutation of [0, P); should a look-back of it ever overrun, its holes must not become addresses)
        const uint32_t row = min(order[i], (uint32_t)(P - 1));
        const float* q = pts + (size_t)row * 3;
        const float x = q[0], y = q[1], z = q[2];
        sorted[i] = make_float4(x, y, z, __uint_as_float(row));
        lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = wave_shfl_min(lo[k]); hi[k] = wave_shfl_max(hi[k]); }
    if (lane == 0) {
        leafbox[2 * (size_t)leaf] = make_float4(lo[0], lo[1], lo[2], 0.f);
        leafbox[2 * (size_t)leaf + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

// one wave per top box: the union of (up to) 64 leaf boxes
__global__ __launch_bounds__(64) void knn_top_kernel(int L, const float4* __restrict__ leafbox, float4* __restrict__ topbox)
{
    const int lane = threadIdx.x;
    const int l = blockIdx.x * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (l < L) { lo = leafbox[2 * (size_t)l]; hi = leafbox[2 * (size_t)l + 1]; }
    lo.x = wave_shfl_min(lo.x); lo.y = wave_shfl_min(lo.y); lo.z = wave_shfl_min(lo.z);
    hi.x = wave_shfl_max(hi.x); hi.y = wave_shfl_max(hi.y); hi.z = wave_shfl_max(hi.z);
    if (lane == 0) { topbox[2 * (size_t)blockIdx.x] = lo; topbox[2 * (size_t)blockIdx.x + 1] = hi; }
}

__device__ __forceinline__ float lane_f(float v, int j)          // v of lane j (j wave-uniform) as a scalar
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
}

// squared distance from p to the box, in the candidates' own arithmetic (see the file header: never above a candidate's distance)
__device__ __forceinline__ float box_point(float lx, float ly, float lz, float hx, float hy, float hz, float px, float py, float pz)
{
    const float ex = fmaxf(fmaxf(lx - px, px - hx), 0.f), ey = fmaxf(fmaxf(ly - py, py - hy), 0.f), ez = fmaxf(fmaxf(lz - pz, pz - hz), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}
// squared distance between two boxes: never above box_point of a point of the one and the other
__device__ __forceinline__ float box_box(const float4 alo, const float4 ahi, const float4 blo, const float4 bhi)
{
    const float gx = fmaxf(fmaxf(blo.x - ahi.x, alo.x - bhi.x), 0.f), gy = fmaxf(fmaxf(blo.y - ahi.y, alo.y - bhi.y), 0.f),
                gz = fmaxf(fmaxf(blo.z - ahi.z, alo.z - bhi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// one candidate (lane j of c) against every lane's query; OWN: candidate j IS query j
template <bool OWN>
__device__ __forceinline__ void knn_candidate(const float4 c, int j, int lane, float px, float py, float pz, float& b0, float& b1, float& b2)
{
    const float dx = px - lane_f(c.x, j), dy = py - lane_f(c.y, j), dz = pz - lane_f(c.z, j);
    float d = (dx * dx + dy * dy) + dz * dz;
    if (OWN && j == lane) d = FLT_MAX;                  // "other" is decided by index, never by distance
    // b0 <= b1 <= b2 stay sorted: min(b1, max(b0, d)) is the median of (b0, b1, d)
    const float n1 = __builtin_amdgcn_fmed3f(b0, b1, d), n2 = __builtin_amdgcn_fmed3f(b1, b2, d);
    b0 = fminf(b0, d); b1 = n1; b2 = n2;
}

// every lane's three smallest values over the candidates held one per lane in c (lanes [0, cnt)).  A full leaf -- all but the last --
// takes the loop of constant length, which unrolls (a loop of v_readlane with a run-time length does not: the operation is convergent).
template <bool OWN>
__device__ __forceinline__ void knn_tile(const float4 c, int cnt, int lane, float px, float py, float pz, float& b0, float& b1, float& b2)
{
    if (cnt == 64) {
#pragma unroll 16
        for (int j = 0; j < 64; ++j) knn_candidate<OWN>(c, j, lane, px, py, pz, b0, b1, b2);
    } else {
#pragma unroll 1
        for (int j = 0; j < cnt; ++j) knn_candidate<OWN>(c, j, lane, px, py, pz, b0, b1, b2);
    }
}

__global__ __launch_bounds__(64 * KNN_WAVES) void knn_search_kernel(int P, int L, int T, const float4* __restrict__ sorted,
                                                                    const float4* __restrict__ leafbox, const float4* __restrict__ topbox,
                                                                    float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int leaf = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * KNN_WAVES + (threadIdx.x >> 6)));     // wave-uniform; no workgroup barrier below
    if (leaf >= L) return;
    const int base = leaf * 64;
    const int cnt = min(64, P - base);
    const bool valid = lane < cnt;
    const float4 me = sorted[base + min(lane, cnt - 1)];              // lanes past the end repeat the last point and write nothing
    const float px = me.x, py = me.y, pz = me.z;
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    knn_tile<true>(me, cnt, lane, px, py, pz, b0, b1, b2);
    if (leaf > 0) knn_tile<false>(sorted[base - 64 + lane], 64, lane, px, py, pz, b0, b1, b2);
    if (leaf + 1 < L) {
        const int ncnt = min(64, P - (base + 64));
        knn_tile<false>(sorted[base + 64 + min(lane, ncnt - 1)], ncnt, lane, px, py, pz, b0, b1, b2);
    }
    float R = wave_shfl_max(valid ? b2 : 0.f);                           // no lane of the wave needs anything at this distance or beyond
    const float4 qlo = leafbox[2 * (size_t)leaf], qhi = leafbox[2 * (size_t)leaf + 1];
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        bool hit = false;
        if (t < T) hit = box_box(qlo, qhi, topbox[2 * (size_t)t], topbox[2 * (size_t)t + 1]) < R;
        uint64_t mt = __builtin_amdgcn_ballot_w64(hit);
        while (mt != 0ull) {
            const int tt = t0 + __builtin_ctzll(mt);
            mt &= mt - 1ull;
            const int l = tt * 64 + lane;
            float4 llo = make_float4(0.f, 0.f, 0.f, 0.f), lhi = llo;
            bool lh = false;
            if (l < L && (l < leaf - 1 || l > leaf + 1)) {            // (the seed has taken the three leaves around the wave's own)
                llo = leafbox[2 * (size_t)l]; lhi = leafbox[2 * (size_t)l + 1];
                lh = box_box(qlo, qhi, llo, lhi) < R;
            }
            uint64_t ml = __builtin_amdgcn_ballot_w64(lh);
            while (ml != 0ull) {
                const int k = __builtin_ctzll(ml);
                ml &= ml - 1ull;
                // (the cross-lane reads stay outside the && : every lane takes part in them)
                const float bp = box_point(lane_f(llo.x, k), lane_f(llo.y, k), lane_f(llo.z, k), lane_f(lhi.x, k), lane_f(lhi.y, k),
                                           lane_f(lhi.z, k), px, py, pz);
                if (__builtin_amdgcn_ballot_w64(valid && bp < b2) == 0ull) continue;
                const int cbase = (tt * 64 + k) * 64;
                const int ccnt = min(64, P - cbase);
                knn_tile<false>(sorted[cbase + min(lane, ccnt - 1)], ccnt, lane, px, py, pz, b0, b1, b2);
                R = wave_shfl_max(valid ? b2 : 0.f);
            }
        }
    }
    if (valid) out[__float_as_uint(me.w)] = ((b0 + b1) + b2) / 3.0f;
}

}  // namespace

size_t mrgs_knn_ws_bytes(int64_t P)
{
    if (P < 0 || P >= ((int64_t)1 << 31)) return 0;
    return knn_ws(P).total;
}

int mrgs_knn_mean_dist2(const float* points, int64_t P, float* out, void* ws, size_t ws_bytes, void* stream)
{
    if (P < 0 || P >= ((int64_t)1 << 31)) return MRGS_E_BAD_ARG;
    if (P == 0) return MRGS_OK;
    if (!points || !out || !ws || ((uintptr_t)ws & 15u) != 0) return MRGS_E_BAD_ARG;
    const KnnWs w = knn_ws(P);
    if (ws_bytes < w.total) return MRGS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    const int n = (int)P, L = (int)w.L, T = (int)w.T;
    MRGS_HIP_TRY(hipMemsetAsync(base + w.zero_from, 0, w.zero_bytes, st));
    uint32_t* bounds = (uint32_t*)(base + w.bounds);
    uint32_t* key[2] = {(uint32_t*)(base + w.key0), (uint32_t*)(base + w.key1)};
    uint32_t* val[2] = {(uint32_t*)(base + w.val0), (uint32_t*)(base + w.val1)};
    float4* sorted = (float4*)(base + w.sorted);
    float4* leafbox = (float4*)(base + w.leafbox);
    float4* topbox = (float4*)(base + w.topbox);
    const unsigned nb = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(knn_bounds_kernel, dim3(nb < (unsigned)KNN_BOUNDS_BLOCKS ? nb : (unsigned)KNN_BOUNDS_BLOCKS), dim3(256), 0, st, n, points,
                       bounds + 16, bounds + 9, bounds);
    hipLaunchKernelGGL(knn_morton_kernel, dim3(nb), dim3(256), 0, st, n, points, bounds, key[0], val[0]);
    const int cur = mrgs_radix_sort_pairs(key, val, (uint32_t*)(base + w.sortws), bounds + 8, P, nullptr, 0, 30, st);
    const unsigned lb = (unsigned)((L + KNN_WAVES - 1) / KNN_WAVES);
    hipLaunchKernelGGL(knn_gather_kernel, dim3(lb), dim3(64 * KNN_WAVES), 0, st, n, L, points, val[cur], sorted, leafbox);
    hipLaunchKernelGGL(knn_top_kernel, dim3((unsigned)T), dim3(64), 0, st, L, leafbox, topbox);
    hipLaunchKernelGGL(knn_search_kernel, dim3(lb), dim3(64 * KNN_WAVES), 0, st, n, L, T, sorted, leafbox, topbox, out);
    return MRGS_LAUNCH_STATUS();
}
