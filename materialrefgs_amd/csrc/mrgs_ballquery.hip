// mrgs_ballquery.hip -- pointnet2_ops' ball_query and furthest_point_sample, and the 3D max-pooling of the reflection score built on them.
//
// Replaces `from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample` at the top of the reference's
// utils/ref_score_utils.py (a CUDA-only extension that is not part of the reference's tree) and the body of that file's
// ref_scores_max_pooling / ref_scores_max_pooling_wiht_mask.  pointnet2_ops' source is not vendored anywhere: the semantics below restate
// its published kernels (ball_query.cu: query_ball_point_kernel; sampling.cu: furthest_point_sampling_kernel), and they -- not a binary --
// are what is pinned (tests/pool_statement.py).  Parity with the CUDA binary is unpinned; nvcc contracts a*b+c by default, so its
// distances may differ from these in the last bit, and a point at the rim of a ball may fall on the other side.
//
//   d(q, k) = (dx dx + dy dy) + dz dz in fp32, un-fused (this file is compiled with -ffp-contract=off), dx = fl(q.x - p_k.x), ...
//   r = (float)radius, r2 = fl(r r); k is a HIT of q iff d(q, k) < r2, strictly.  A comparison with a NaN is false: a row with a
//   non-finite coordinate never hits and is never hit.
//
//   ball_query(radius, nsample, xyz [B,N,3], new_xyz [B,M,3]) -> int32 [B,M,nsample]: with h_0 < h_1 < ... the hits of query j in
//   ascending index order and c = min(#hits, nsample), row j is h_0 .. h_{c-1} followed by h_0 repeated; a row without hits is all zeros.
//   A pure function of the inputs, bit-equal to the fp32 brute force over k = 0 .. N-1.
//
//   furthest_point_sample(xyz [B,N,3], npoint) -> int32 [B,npoint]: idx[0] = 0, temp[k] = 1e10.  For each further pick every k whose
//   magnitude (x x + y y) + z z (fp32, un-fused) is > 1e-3 (the comparison in double, as the published kernel's `mag <= 1e-3` skip) is
//   ELIGIBLE and takes temp[k] = fminf(temp[k], d(p_old, p_k)), p_old the pick before; the pick is the eligible k of largest temp[k],
//   ties to the LOWEST index (this project's rule: the CUDA kernel's tie depends on its block size); no eligible point: the pick is 0.
//   The magnitude test is the published kernel's and is kept: points within 0.0316 of the origin are never picked after idx[0].
//
//   pooled[j] = the maximum (fmaxf: first hit's score, then fmaxf with each further one) of score[k] over the row ball_query(r, nsample,
//   points, points) would give for j -- the first nsample hits in index order, not all hits.  Without a validity mask a row without hits
//   takes score[0], as the zero row does.  With one, rows whose mask is zero are neither candidates nor queries and keep their own
//   score, the order among the others is their order in the full cloud, and a masked-in row without a hit keeps its own score.
//
// Everything below only prunes.  "First hits in ascending index order" fixes the order of the walk, so the hierarchy is built over the
// ORIGINAL order and nothing is sorted: a LEAF box covers 64 consecutive points, a TOP box 64 consecutive leaves; rows with a non-finite
// coordinate (and masked-out rows) are left out of the boxes.  A depth-map cloud is image-ordered -- consecutive indices are neighbours in
// space -- so its boxes are tight; for an unordered cloud they are loose and only the speed suffers.
//   bq_leaf_kernel   one wave per leaf: packed[i] = (x, y, z, score or 0) as 16-byte rows (x = NaN for a masked-out row) and the leaf's box
//   bq_top_kernel    one wave per top box: the union of (up to) 64 leaf boxes
//   bq_walk_kernel   the shape of knn_search_kernel (mrgs_knn.hip): one wave per 64 consecutive queries, one per lane.  Top boxes in
//                    ascending order, 64 a step, each lane testing a DIFFERENT box against the wave's query box; survivors in ascending
//                    bit order of the ballot; the 64 leaves of a surviving top box the same way; per surviving leaf a wave-uniform test
//                    whether any unfinished lane's ball meets the leaf box; if one does, one coalesced 1 KB load of the leaf's 64 packed
//                    candidates, handed round with v_readlane, every lane appending its hits in order.  A lane is finished at nsample
//                    hits; the wave leaves when all its lanes are finished or the boxes are exhausted: every loop is bounded by a box count.
//                    Two instances: INDICES (a row's hits go to memory as they are found -- 49 indices do not live in registers -- the
//                    padding when the lane is done) and POOLED (a running maximum and a count; the queries are the packed rows
//                    themselves; no index exists anywhere).
//   bq_points_kernel all views' points from their depth maps and a per-view camera table, x and y from the thread index
//   bq_fps_kernel    one launch per pick: temp update, per-block argmax partials, the last block folds them and writes the pick, which
//                    the next launch reads from device memory (no host read)
// Pruning is exact in fp32 by the argument of mrgs_knn.hip: for a candidate c inside a box, |fl(q - c)| >= fl(gap to the box) per axis
// (rounding is monotonic), and the squares and the two sums are monotonic too when taken in the same order, so box distance <= candidate
// distance AS COMPUTED; a box whose distance is not < r2 holds no hit.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "mrgs_internal.h"
#include "mrgs_wave.h"

#define BQ_LAUNCH_STATUS mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__)

namespace {

constexpr int BQ_WAVES = 4;                  // waves per workgroup of the leaf build and the walk
constexpr int BQ_FPS_BLOCKS = 256;           // at most this many partial rows per batch and pick

struct BqWs {
    size_t packed, leafbox, topbox, total;                   // the walk
    size_t temp, partial, ticket;                            // furthest point sampling (shares the bytes)
    int64_t L, T;
};

BqWs bq_ws(int64_t B, int64_t N)
{
    BqWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = mrgs_align_up(o + bytes, 256); return at; };
    w.L = (N + 63) / 64;
    w.T = (w.L + 63) / 64;
    w.packed = take((size_t)B * N * 16);
    w.leafbox = take((size_t)B * w.L * 32);                  // (lo.xyz, -) (hi.xyz, -)
    w.topbox = take((size_t)B * w.T * 32);
    const size_t walk = o;
    o = 0;
    w.temp = take((size_t)B * N * 4);
    w.partial = take((size_t)B * BQ_FPS_BLOCKS * 8);
    w.ticket = take((size_t)B * 4);
    w.total = walk > o ? walk : o;
    return w;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

// one wave per leaf of batch blockIdx.y: the packed rows and the box of the rows that can hit
__global__ __launch_bounds__(64 * BQ_WAVES) void bq_leaf_kernel(int N, int L, const float* __restrict__ xyz, const float* __restrict__ score,
                                                                const uint8_t* __restrict__ valid, float4* __restrict__ packed,
                                                                float4* __restrict__ leafbox)
{
    const int lane = threadIdx.x & 63;
    const int leaf = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * BQ_WAVES + (threadIdx.x >> 6)));
    if (leaf >= L) return;
    const size_t b = blockIdx.y;
    const int64_t i = (int64_t)leaf * 64 + lane;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < N) {
        const size_t row = b * (size_t)N + (size_t)i;
        const float* q = xyz + row * 3;
        float x = q[0];
        const float y = q[1], z = q[2];
        if (valid && valid[row] == 0) x = NAN;                        // neither a candidate nor a query
        packed[row] = make_float4(x, y, z, score ? score[row] : 0.f);
        if (finite3(x, y, z)) { lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = wave_shfl_min(lo[k]); hi[k] = wave_shfl_max(hi[k]); }
    if (lane == 0) {
        leafbox[2 * (b * (size_t)L + leaf)] = make_float4(lo[0], lo[1], lo[2], 0.f);
        leafbox[2 * (b * (size_t)L + leaf) + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

// one wave per top box of batch blockIdx.y
__global__ __launch_bounds__(64) void bq_top_kernel(int L, int T, const float4* __restrict__ leafbox, float4* __restrict__ topbox)
{
    const int lane = threadIdx.x;
    const size_t b = blockIdx.y;
    const int l = blockIdx.x * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (l < L) { lo = leafbox[2 * (b * (size_t)L + l)]; hi = leafbox[2 * (b * (size_t)L + l) + 1]; }
    lo.x = wave_shfl_min(lo.x); lo.y = wave_shfl_min(lo.y); lo.z = wave_shfl_min(lo.z);
    hi.x = wave_shfl_max(hi.x); hi.y = wave_shfl_max(hi.y); hi.z = wave_shfl_max(hi.z);
    if (lane == 0) { topbox[2 * (b * (size_t)T + blockIdx.x)] = lo; topbox[2 * (b * (size_t)T + blockIdx.x) + 1] = hi; }
}

__device__ __forceinline__ float lane_f(float v, int j)          // v of lane j (j wave-uniform) as a scalar
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j));
}

// squared distance from p to the box, in the candidates' own arithmetic (see the file header: never above a candidate's distance);
// an empty box (lo = +inf, hi = -inf) is at +inf
__device__ __forceinline__ float box_point(float lx, float ly, float lz, float hx, float hy, float hz, float px, float py, float pz)
{
    const float ex = fmaxf(fmaxf(lx - px, px - hx), 0.f), ey = fmaxf(fmaxf(ly - py, py - hy), 0.f), ez = fmaxf(fmaxf(lz - pz, pz - hz), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}
// squared distance between two boxes: never above box_point of a point of the one and the other
__device__ __forceinline__ float box_box(float alx, float aly, float alz, float ahx, float ahy, float ahz, const float4 blo, const float4 bhi)
{
    const float gx = fmaxf(fmaxf(blo.x - ahx, alx - bhi.x), 0.f), gy = fmaxf(fmaxf(blo.y - ahy, aly - bhi.y), 0.f),
                gz = fmaxf(fmaxf(blo.z - ahz, alz - bhi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// What a lane keeps of its row.  INDICES: where the row goes, and h_0 for the padding.  POOLED: the running maximum.
template <bool POOLED>
struct BqRow {
    int cnt;
    int first;
    float best;
    int32_t* out;
};

// one candidate (lane j of c, index kbase + j) against every lane's query
template <bool POOLED>
__device__ __forceinline__ void bq_candidate(const float4 c, int j, int kbase, float qx, float qy, float qz, float r2, int nsample, BqRow<POOLED>& row)
{
    const float dx = qx - lane_f(c.x, j), dy = qy - lane_f(c.y, j), dz = qz - lane_f(c.z, j);
    const float d = (dx * dx + dy * dy) + dz * dz;
    const float s = POOLED ? lane_f(c.w, j) : 0.f;                 // (the cross-lane read stays outside the branch)
    if (d < r2 && row.cnt < nsample) {
        if (POOLED) {
            row.best = row.cnt == 0 ? s : fmaxf(row.best, s);
        } else {
            if (row.cnt == 0) row.first = kbase + j;
            row.out[row.cnt] = kbase + j;
        }
        ++row.cnt;
    }
}

// the candidates held one per lane in c (lanes [0, ccnt)), in ascending order.  A full leaf -- all but the last -- takes the loop of
// constant length, which unrolls (a loop of v_readlane with a run-time length does not: the operation is convergent).
template <bool POOLED>
__device__ __forceinline__ void bq_tile(const float4 c, int ccnt, int kbase, float qx, float qy, float qz, float r2, int nsample, BqRow<POOLED>& row)
{
    if (ccnt == 64) {
#pragma unroll 8
        for (int j = 0; j < 64; ++j) bq_candidate<POOLED>(c, j, kbase, qx, qy, qz, r2, nsample, row);
    } else {
#pragma unroll 1
        for (int j = 0; j < ccnt; ++j) bq_candidate<POOLED>(c, j, kbase, qx, qy, qz, r2, nsample, row);
    }
}

// INDICES: queries [B,M,3], idx [B,M,nsample].  POOLED: the queries are the packed rows (M = N), pooled [B,N]; own_on_empty: a row without
// a hit keeps its own score (the masked variant), otherwise it takes score[0] of its batch.
// r = radius_dev ? fl(*radius_dev * radius) : radius.
template <bool POOLED>
__global__ __launch_bounds__(64 * BQ_WAVES) void bq_walk_kernel(int N, int M, int L, int T, int nsample, float radius, const float* __restrict__ radius_dev,
                                                                const float4* __restrict__ packed, const float4* __restrict__ leafbox,
                                                                const float4* __restrict__ topbox, const float* __restrict__ queries,
                                                                int32_t* __restrict__ idx, float* __restrict__ pooled, int own_on_empty)
{
    const int lane = threadIdx.x & 63;
    const int group = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * BQ_WAVES + (threadIdx.x >> 6)));   // wave-uniform; no workgroup barrier below
    const int64_t qbase = (int64_t)group * 64;
    if (qbase >= M) return;
    const size_t b = blockIdx.y;
    const float r = radius_dev ? *radius_dev * radius : radius;
    const float r2 = r * r;
    const int64_t qi = qbase + lane;
    const bool inrange = qi < M;                                    // lanes past the end stay in the wave (cross-lane reads) and write nothing
    float qx = NAN, qy = NAN, qz = NAN, qs = 0.f;
    if (inrange) {
        if (POOLED) {
            const float4 me = packed[b * (size_t)N + (size_t)qi];
            qx = me.x; qy = me.y; qz = me.z; qs = me.w;
        } else {
            const float* q = queries + (b * (size_t)M + (size_t)qi) * 3;
            qx = q[0]; qy = q[1]; qz = q[2];
        }
    }
    const bool live = inrange && finite3(qx, qy, qz);               // a query that can hit at all
    // the wave's query box (uniform values)
    const float alx = wave_dpp_min(live ? qx : INFINITY), aly = wave_dpp_min(live ? qy : INFINITY), alz = wave_dpp_min(live ? qz : INFINITY);
    const float ahx = wave_dpp_max(live ? qx : -INFINITY), ahy = wave_dpp_max(live ? qy : -INFINITY), ahz = wave_dpp_max(live ? qz : -INFINITY);
    BqRow<POOLED> row;
    row.cnt = 0; row.first = 0; row.best = 0.f;
    row.out = POOLED ? nullptr : idx + (b * (size_t)M + (size_t)(inrange ? qi : 0)) * (size_t)nsample;
    const float4* lbox = leafbox + 2 * b * (size_t)L;
    const float4* tbox = topbox + 2 * b * (size_t)T;
    const float4* cand = packed + b * (size_t)N;
    uint64_t unfinished = __builtin_amdgcn_ballot_w64(live);
    for (int t0 = 0; t0 < T && unfinished != 0ull; t0 += 64) {
        const int t = t0 + lane;
        bool th = false;
        if (t < T) th = box_box(alx, aly, alz, ahx, ahy, ahz, tbox[2 * (size_t)t], tbox[2 * (size_t)t + 1]) < r2;
        uint64_t mt = __builtin_amdgcn_ballot_w64(th);
        while (mt != 0ull && unfinished != 0ull) {
            const int tt = t0 + __builtin_ctzll(mt);
            mt &= mt - 1ull;
            const int l = tt * 64 + lane;
            float4 llo = make_float4(0.f, 0.f, 0.f, 0.f), lhi = llo;
            bool lh = false;
            if (l < L) {
                llo = lbox[2 * (size_t)l]; lhi = lbox[2 * (size_t)l + 1];
                lh = box_box(alx, aly, alz, ahx, ahy, ahz, llo, lhi) < r2;
            }
            uint64_t ml = __builtin_amdgcn_ballot_w64(lh);
            while (ml != 0ull && unfinished != 0ull) {
                const int k = __builtin_ctzll(ml);
                ml &= ml - 1ull;
                // (the cross-lane reads stay outside the && : every lane takes part in them)
                const float bp = box_point(lane_f(llo.x, k), lane_f(llo.y, k), lane_f(llo.z, k), lane_f(lhi.x, k), lane_f(lhi.y, k),
                                           lane_f(lhi.z, k), qx, qy, qz);
                if (__builtin_amdgcn_ballot_w64(live && row.cnt < nsample && bp < r2) == 0ull) continue;
                const int64_t cbase = ((int64_t)tt * 64 + k) * 64;                 // < N: the leaf exists
                const int ccnt = (int)(N - cbase < 64 ? N - cbase : 64);
                bq_tile<POOLED>(cand[(size_t)cbase + min(lane, ccnt - 1)], ccnt, (int)cbase, qx, qy, qz, r2, nsample, row);
                unfinished = __builtin_amdgcn_ballot_w64(live && row.cnt < nsample);
            }
        }
    }
    if (!inrange) return;
    if (POOLED) {
        float v = row.best;
        if (row.cnt == 0) v = own_on_empty ? qs : cand[0].w;
        pooled[b * (size_t)N + (size_t)qi] = v;
    } else {
        for (int p = row.cnt; p < nsample; ++p) row.out[p] = row.first;             // h_0 repeated; no hit: zeros
    }
}

// point (v H W + y W + x) of view v: ((x - Cx) / Fx z, (y - Cy) / Fy z, z) with z the depth, then (p - T) @ R^T
__global__ __launch_bounds__(256) void bq_points_kernel(int H, int W, const MrgsDepthView* __restrict__ views, float* __restrict__ points)
{
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    if (pix >= HW) return;
    const MrgsDepthView* v = views + blockIdx.y;
    const int y = (int)(pix / W), x = (int)(pix - (int64_t)y * W);
    const float z = v->depth[pix];
    const float px = ((float)x - v->cx) / v->fx * z, py = ((float)y - v->cy) / v->fy * z;
    const float d0 = px - v->T[0], d1 = py - v->T[1], d2 = z - v->T[2];
    float* o = points + ((size_t)blockIdx.y * (size_t)HW + (size_t)pix) * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (d0 * v->R[3 * i] + d1 * v->R[3 * i + 1]) + d2 * v->R[3 * i + 2];
}

__device__ __forceinline__ unsigned long long ld_agent64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long wave_shfl_max64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long n = __shfl_xor(v, o, 64);
        v = n > v ? n : v;
    }
    return v;
}

// Pick `pick` (>= 1) of batch blockIdx.y.  A thread's key is (bits of temp[k]) << 32 | ~k for its best eligible k (temp >= 0, never NaN:
// its bits order as the values; ~k: the lowest index wins a tie) and 0 without one; per-block partial keys, the last block to finish
// folds them (the ticket of grid_max6_last_block_folds), writes idx[pick] and clears the ticket for the next launch.  With span_out and
// pick == 1 it also writes |p[idx[0]] - p[idx[1]]| (the square root correctly rounded: taken in double).
__global__ __launch_bounds__(256) void bq_fps_kernel(int N, int npoint, int pick, const float* __restrict__ xyz, float* __restrict__ temp,
                                                     unsigned long long* __restrict__ partial, uint32_t* __restrict__ ticket,
                                                     int32_t* __restrict__ idx, float* __restrict__ span_out)
{
    __shared__ unsigned long long red[4];
    __shared__ bool last;
    const size_t b = blockIdx.y;
    const float* pts = xyz + b * (size_t)N * 3;
    float* tmp = temp + b * (size_t)N;
    int32_t* row = idx + b * (size_t)npoint;
    int old = pick == 1 ? 0 : row[pick - 1];
    old = min(max(old, 0), N - 1);                                   // (written by the launch before: always inside; an address all the same)
    const float ox = pts[(size_t)old * 3], oy = pts[(size_t)old * 3 + 1], oz = pts[(size_t)old * 3 + 2];
    unsigned long long best = 0ull;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < N; k += (int64_t)gridDim.x * 256) {
        const float x = pts[(size_t)k * 3], y = pts[(size_t)k * 3 + 1], z = pts[(size_t)k * 3 + 2];
        const float mag = (x * x + y * y) + z * z;
        if (!((double)mag > 1e-3)) continue;
        const float dx = ox - x, dy = oy - y, dz = oz - z;
        const float t = fminf(pick == 1 ? 1e10f : tmp[k], (dx * dx + dy * dy) + dz * dz);
        tmp[k] = t;
        const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)(~(uint32_t)k);
        best = key > best ? key : best;
    }
    best = wave_shfl_max64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = red[0];
        for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
        st_agent64(partial + b * BQ_FPS_BLOCKS + blockIdx.x, m);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket + b, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    unsigned long long mine = threadIdx.x < gridDim.x ? ld_agent64(partial + b * BQ_FPS_BLOCKS + threadIdx.x) : 0ull;   // gridDim.x <= 256
    mine = wave_shfl_max64(mine);
    __syncthreads();                                                 // `red` is reused
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = red[0];
        for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
        const int chosen = m != 0ull ? (int)(~(uint32_t)m) : 0;
        row[pick] = chosen;
        st_agent(ticket + b, 0u);
        if (span_out && pick == 1) {
            const float dx = pts[0] - pts[(size_t)chosen * 3], dy = pts[1] - pts[(size_t)chosen * 3 + 1], dz = pts[2] - pts[(size_t)chosen * 3 + 2];
            span_out[b] = (float)sqrt((double)((dx * dx + dy * dy) + dz * dz));
        }
    }
}

bool bq_sizes_ok(int64_t B, int64_t N) { return B >= 0 && B <= 65535 && N >= 0 && N < ((int64_t)1 << 31); }

// the hierarchy over xyz [B,N,3] (score, valid optional) into the workspace
int bq_build(const BqWs& w, char* base, int64_t B, int64_t N, const float* xyz, const float* score, const uint8_t* valid, hipStream_t st)
{
    const unsigned lb = (unsigned)((w.L + BQ_WAVES - 1) / BQ_WAVES);
    hipLaunchKernelGGL(bq_leaf_kernel, dim3(lb, (unsigned)B), dim3(64 * BQ_WAVES), 0, st, (int)N, (int)w.L, xyz, score, valid,
                       (float4*)(base + w.packed), (float4*)(base + w.leafbox));
    hipLaunchKernelGGL(bq_top_kernel, dim3((unsigned)w.T, (unsigned)B), dim3(64), 0, st, (int)w.L, (int)w.T, (const float4*)(base + w.leafbox),
                       (float4*)(base + w.topbox));
    return BQ_LAUNCH_STATUS;
}

}  // namespace

size_t mrgs_ball_query_ws_bytes(int64_t B, int64_t N)
{
    if (!bq_sizes_ok(B, N)) return 0;
    return bq_ws(B, N).total;
}

int mrgs_ball_query(float radius, int32_t nsample, const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t M, int32_t* idx, void* ws,
                    size_t ws_bytes, void* stream)
{
    if (!bq_sizes_ok(B, N) || M < 0 || M >= ((int64_t)1 << 31) || nsample < 1) return MRGS_E_BAD_ARG;
    if (B == 0 || M == 0) return MRGS_OK;
    if (!idx || !new_xyz || (N > 0 && (!xyz || !ws || ((uintptr_t)ws & 15u) != 0))) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                                                    // no candidate: every row is zeros
        MRGS_HIP_TRY(hipMemsetAsync(idx, 0, (size_t)B * M * nsample * 4, st));
        return MRGS_OK;
    }
    const BqWs w = bq_ws(B, N);
    if (ws_bytes < w.total) return MRGS_E_WORKSPACE;
    char* base = (char*)ws;
    if (int rc = bq_build(w, base, B, N, xyz, nullptr, nullptr, st)) return rc;
    const unsigned qb = (unsigned)((M + 64 * BQ_WAVES - 1) / (64 * BQ_WAVES));
    hipLaunchKernelGGL(bq_walk_kernel<false>, dim3(qb, (unsigned)B), dim3(64 * BQ_WAVES), 0, st, (int)N, (int)M, (int)w.L, (int)w.T, nsample, radius,
                       (const float*)nullptr, (const float4*)(base + w.packed), (const float4*)(base + w.leafbox), (const float4*)(base + w.topbox),
                       new_xyz, idx, (float*)nullptr, 0);
    return BQ_LAUNCH_STATUS;
}

int mrgs_ball_max_pool(float radius, const float* radius_dev, int32_t nsample, const float* points, const float* score, const uint8_t* valid, int64_t B,
                       int64_t N, float* pooled, void* ws, size_t ws_bytes, void* stream)
{
    if (!bq_sizes_ok(B, N) || nsample < 1) return MRGS_E_BAD_ARG;
    if (B == 0 || N == 0) return MRGS_OK;
    if (!points || !score || !pooled || !ws || ((uintptr_t)ws & 15u) != 0) return MRGS_E_BAD_ARG;
    const BqWs w = bq_ws(B, N);
    if (ws_bytes < w.total) return MRGS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    if (int rc = bq_build(w, base, B, N, points, score, valid, st)) return rc;
    const unsigned qb = (unsigned)((N + 64 * BQ_WAVES - 1) / (64 * BQ_WAVES));
    hipLaunchKernelGGL(bq_walk_kernel<true>, dim3(qb, (unsigned)B), dim3(64 * BQ_WAVES), 0, st, (int)N, (int)N, (int)w.L, (int)w.T, nsample, radius,
                       radius_dev, (const float4*)(base + w.packed), (const float4*)(base + w.leafbox), (const float4*)(base + w.topbox),
                       (const float*)nullptr, (int32_t*)nullptr, pooled, valid ? 1 : 0);
    return BQ_LAUNCH_STATUS;
}

int mrgs_furthest_point_sample(const float* xyz, int64_t B, int64_t N, int32_t npoint, int32_t* idx, float* span_out, void* ws, size_t ws_bytes,
                               void* stream)
{
    if (!bq_sizes_ok(B, N) || npoint < 0) return MRGS_E_BAD_ARG;
    if (B == 0 || npoint == 0) return MRGS_OK;
    if (N == 0 || !xyz || !idx || !ws || ((uintptr_t)ws & 15u) != 0) return MRGS_E_BAD_ARG;       // a pick needs a point
    const BqWs w = bq_ws(B, N);
    if (ws_bytes < w.total) return MRGS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    MRGS_HIP_TRY(hipMemsetAsync(idx, 0, (size_t)B * npoint * 4, st));                             // idx[0] = 0
    MRGS_HIP_TRY(hipMemsetAsync(base + w.ticket, 0, (size_t)B * 4, st));
    if (span_out && npoint < 2) MRGS_HIP_TRY(hipMemsetAsync(span_out, 0, (size_t)B * 4, st));    // no second pick: the span is 0
    const int64_t nb = (N + 255) / 256;
    const unsigned blocks = (unsigned)(nb < BQ_FPS_BLOCKS ? nb : BQ_FPS_BLOCKS);
    for (int pick = 1; pick < npoint; ++pick)
        hipLaunchKernelGGL(bq_fps_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, st, (int)N, (int)npoint, pick, xyz, (float*)(base + w.temp),
                           (unsigned long long*)(base + w.partial), (uint32_t*)(base + w.ticket), idx, span_out);
    return BQ_LAUNCH_STATUS;
}

int mrgs_depth_points(const MrgsDepthView* views, int32_t n_views, int32_t H, int32_t W, float* points, void* stream)
{
    if (n_views < 0 || n_views > 65535 || H < 0 || W < 0) return MRGS_E_BAD_ARG;
    const int64_t HW = (int64_t)H * W;
    if (HW * (int64_t)n_views >= ((int64_t)1 << 31)) return MRGS_E_BAD_ARG;
    if (n_views == 0 || HW == 0) return MRGS_OK;
    if (!views || !points) return MRGS_E_BAD_ARG;
    hipLaunchKernelGGL(bq_points_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)n_views), dim3(256), 0, (hipStream_t)stream, (int)H, (int)W, views,
                       points);
    return BQ_LAUNCH_STATUS;
}
