// mrgs_wave.h -- wave64 and workgroup primitives shared by the kernel files: each exists here once.
//
// Wave reductions, the workgroup scans (of one value per thread, and of a whole array of per-workgroup counts by one workgroup), the packed
// triple of counts that travels through those scans, the partial-row sums of the per-view term kernels, and the last-block fold of six maxima.
//
// Two families of wave-wide reductions, told apart by name:
//   wave_shfl_*   __shfl_xor butterfly: six ds_bpermute round trips through the LDS crossbar, the result in EVERY lane (a vector register)
//   wave_dpp_*    six DPP steps on the VALU, the result read from lane 63 and therefore wave-uniform (a scalar register)
// The values are the same up to the order of a float sum; the cost and the register class of the result are not.
#pragma once
#include "mrgs_internal.h"

// ---- relaxed agent-scope word access (tickets, look-back status words, partial rows another workgroup reads) ----------------------
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- one wave's lanes exchange data through LDS --------------------------------------------------------------------------------------
// What the lanes of this wave wrote to LDS before the call, every lane of it reads behind it (no s_barrier: the other waves of the
// workgroup are not waited for).  So far only the surfel tracer calls it; the other files still spell the three lines out.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- ordered float keys, Morton codes --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ord_f(float f)          // order-preserving float -> uint
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f(uint32_t u)
{
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ uint32_t spread10(uint32_t v)      // 10 bits -> every third bit
{
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// ---- shuffle butterflies: result in every lane, via LDS permute --------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_shfl_sum(T v)               // float or double
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_shfl_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_shfl_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_shfl_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// ---- DPP reductions: result uniform, six DPP steps -----------------------------------------------------------------------------------
// xor 1, xor 2 inside the quads, rotations by 4 and 8 inside the 16-lane rows, then lane 15 / lane 31 of the rows before into the rows
// behind (row_bcast) -- lane 63 ends up with the result of all 64.  Six dependent VALU instructions; a __shfl_xor butterfly goes through
// ds_bpermute, six dependent ~120-cycle LDS round trips (measured in the tracer: a packet wave spends 500 of these reductions a view --
// nearest child, far bound, beams, packet tests -- i.e. ~40 % of its 470 us in them).  Masked-out rows take `old`.  Every lane of the
// wave must be active.
#define MRGS_DPP(OLD, V, CTRL, RM) __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(OLD), __float_as_int(V), CTRL, RM, 0xf, false))
__device__ __forceinline__ float wave_lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
// one step of a DPP sum: v + (v moved by CTRL, 0 where no lane is the source or the row is masked out)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + MRGS_DPP(0.0f, v, CTRL, ROW_MASK);
}
__device__ __forceinline__ float wave_dpp_sum(float v)
{
    v = dpp_add<0xb1, 0xf>(v); v = dpp_add<0x4e, 0xf>(v); v = dpp_add<0x124, 0xf>(v); v = dpp_add<0x128, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v); v = dpp_add<0x143, 0xc>(v);
    return wave_lane63(v);
}
__device__ __forceinline__ float wave_dpp_max(float v)
{
    v = fmaxf(v, MRGS_DPP(v, v, 0xb1, 0xf)); v = fmaxf(v, MRGS_DPP(v, v, 0x4e, 0xf)); v = fmaxf(v, MRGS_DPP(v, v, 0x124, 0xf)); v = fmaxf(v, MRGS_DPP(v, v, 0x128, 0xf));
    v = fmaxf(v, MRGS_DPP(v, v, 0x142, 0xa)); v = fmaxf(v, MRGS_DPP(v, v, 0x143, 0xc));
    return wave_lane63(v);
}
__device__ __forceinline__ float wave_dpp_min(float v)
{
    v = fminf(v, MRGS_DPP(v, v, 0xb1, 0xf)); v = fminf(v, MRGS_DPP(v, v, 0x4e, 0xf)); v = fminf(v, MRGS_DPP(v, v, 0x124, 0xf)); v = fminf(v, MRGS_DPP(v, v, 0x128, 0xf));
    v = fminf(v, MRGS_DPP(v, v, 0x142, 0xa)); v = fminf(v, MRGS_DPP(v, v, 0x143, 0xc));
    return wave_lane63(v);
}

// ---- workgroup scans ---------------------------------------------------------------------------------------------------------------
// v = this thread's count; returns the exclusive prefix over the 256 threads of the workgroup.  One barrier: s_wave must not be written
// again before every wave has read it (the callers scan once per launch).
template <typename T>
__device__ __forceinline__ T block_exclusive_scan_256(T v, T* s_wave /*[4]*/, T& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T n = __shfl_up(inc, o, 64);
        if (lane >= o) inc += n;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T base = 0;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return base + inc - v;
}
// The same for THREADS threads, with a second barrier behind the reads so that the caller may scan again through the same lds_wave_sums
// (the radix passes do), and every wave sums all THREADS / 64 entries instead of its own predecessors.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds_wave_sums /*[THREADS/64]*/, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds_wave_sums[wave] = inc;
    __syncthreads();
    uint32_t wave_off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; w++) {
        uint32_t s = lds_wave_sums[w];
        if (w < wave) wave_off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return wave_off + inc - v;
}
// exclusive scan of n per-workgroup counts by ONE workgroup of THREADS threads: THREADS consecutive words a step (coalesced), the running
// total carried in registers.  out may be null (total only) or alias in, hence no __restrict__: thread t writes only the words
// t + k THREADS, each after it has read it; the one word it reads that is not its own is in[n - 1], by the clamped loads behind the
// tail, and that value is thrown away.  Returns the total in every thread.  Every one-workgroup pass that turns per-block counts into
// offsets (compaction, both densifiers, the mesh, the multi-view sampler) is this.
// Why not the plain loop (v = i < n ? in[i] : 0; scan; store): a lone workgroup has nothing to hide a step's load behind, and
// mesh_scan_kernel, which had its three rows' loads of a step in flight together, lost 3 % of count + emit to it (tools/mesh_time.py,
// figures in DESIGN.md).  So the next step's word is loaded before this step's is scanned.  Seen in the generated code (make
// mrgs_optim.s, compact_scan_kernel): with that load under `if (i + THREADS < n)` an s_waitcnt vmcnt(0) follows it at once; with the
// use of `next` left to the end of the body the wait stands behind the store and covers it too.  Hence the clamped index and the empty
// asm that uses `next` before the store; only this final form was timed.
template <int THREADS>
__device__ __forceinline__ uint32_t block_counts_exclusive_scan(int n, const uint32_t* in, uint32_t* out, uint32_t* lds_wave_sums /*[THREADS/64]*/)
{
    if (n <= 0) return 0u;
    uint32_t carry = 0, v = in[min((int)threadIdx.x, n - 1)];
    if ((int)threadIdx.x >= n) v = 0u;
    for (int i = threadIdx.x; i - (int)threadIdx.x < n; i += THREADS) {
        uint32_t next = in[min(i + THREADS, n - 1)];
        if (i + THREADS >= n) next = 0u;
        uint32_t total;
        const uint32_t pre = block_exclusive_scan<THREADS>(v, lds_wave_sums, total);   // its trailing barrier frees lds_wave_sums for the next step
        asm volatile("" : "+v"(next));              // the load's wait goes here, before the store
        if (out && i < n) out[i] = carry + pre;
        carry += total;
        v = next;
    }
    return carry;
}

// Three counts through one 64-bit scan, FIELD bits each: a workgroup's three totals stay below 2^21 (1024 rows; 12 * 256 triangles).
// The packer takes 64-bit parameters on purpose: with 32-bit ones widened inside, mesh_count_kernel came out with other code.
constexpr int FIELD = 21;
constexpr unsigned long long FIELD_MASK = (1ull << FIELD) - 1;
__device__ __forceinline__ unsigned long long pack_fields(unsigned long long c0, unsigned long long c1, unsigned long long c2)
{
    return c0 | (c1 << FIELD) | (c2 << (2 * FIELD));
}
__device__ __forceinline__ unsigned unpack_field(unsigned long long packed, int k) { return (unsigned)((packed >> (FIELD * k)) & FIELD_MASK); }

// ---- K float sums over a whole grid: one partial row per workgroup, the rows summed in double by one workgroup ---------------------------
// The tail of the per-view term kernels (mrgs_loss, mrgs_prior, mrgs_smooth) and the head of their finalize kernels.  256 threads, no
// atomics, every addition in a fixed order: the terms are run-to-run identical.  `red` is the caller's LDS.
// Users: prior_terms_fwd (workgroup side), smooth_terms_finalize (finalize side).  Four kernels compute exactly this and keep it written out,
// because the compiler turns the call into another instruction stream than the one that was measured (tools/isa_digest.py; same registers):
//   loss_fwd_kernel        one more s_xor of exec around the lane-0 stores, with the row pointer formed before or inside the last branch
//   smooth_terms_fwd       30 instructions fewer, scheduled otherwise; its own form stores each sum right behind its butterfly, and with
//                          that form here prior_terms_fwd comes out 108 instructions longer
//   prior_terms_finalize   same length, the `if (a.surf)` branch behind the barrier laid out the other way round
//   loss_finalize_kernel   also reads four rows a pass and picks columns by channel; even wave_shfl_sum<double> for its butterfly
//                          reschedules it (4 instructions fewer)
// Workgroup side: v[0..K) summed over the wave, then over the four waves as (w0 + w1) + (w2 + w3) into row[0..ROW), entries past K as 0.
template <int K, int ROW>
__device__ __forceinline__ void block_row_sum_256(float (&v)[K], float (&red)[4][ROW], float* row)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_shfl_sum(v[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < ROW) row[tid] = tid < K ? (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]) : 0.f;
}
// Finalize side: the nblocks rows of `partials` ([nblocks][ROW], 16-byte aligned), row b by thread b % 256 in ascending b, then over the
// wave; behind its barrier red[w][k] is wave w's sum of column k and rows_total(red, k) the total.
template <int K, int ROW>
__device__ __forceinline__ void block_rows_sum_256(const float* partials, int nblocks, double (&red)[4][K])
{
    static_assert(ROW % 4 == 0 && K <= ROW, "a row is whole 16-byte words");
    const int tid = threadIdx.x;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int b = tid; b < nblocks; b += 256) {                 // one row per thread and pass
        const float4* p = reinterpret_cast<const float4*>(partials + (size_t)b * ROW);
        float4 r[ROW / 4];
#pragma unroll
        for (int w = 0; w < ROW / 4; ++w) r[w] = p[w];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += reinterpret_cast<const float*>(r)[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_shfl_sum(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
}
template <int K>
__device__ __forceinline__ double rows_total(const double (&red)[4][K], int k) { return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]); }

// ---- six maxima over a whole grid without same-address atomics -----------------------------------------------------------------------
// Tail of a 256-thread kernel whose threads each hold six ordered-uint maxima (ext): every block leaves one partial row, takes a ticket,
// and the last block to finish folds the rows into bounds[0..6).  Same-address atomics serialise at L2 (one per wave cost 0.32 ms at
// 300 k surfels).  gridDim.x <= 256; *ticket starts at 0; partial holds gridDim.x * 6 words.
__device__ __forceinline__ void grid_max6_last_block_folds(const uint32_t (&ext)[6], uint32_t* __restrict__ partial, uint32_t* __restrict__ ticket,
                                                           uint32_t* __restrict__ bounds)
{
    __shared__ uint32_t red[4][6];
    __shared__ bool last;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t m = wave_shfl_max(ext[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = m;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        st_agent(partial + blockIdx.x * 6 + k, max(max(red[0][k], red[1][k]), max(red[2][k], red[3][k])));
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    // thread b folds block b's row (gridDim.x <= 256 = blockDim.x); six dependent loops over 256 agent-scope loads cost 50 us
    uint32_t mine[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) mine[k] = threadIdx.x < gridDim.x ? ld_agent(partial + threadIdx.x * 6 + k) : 0u;
    __syncthreads();                       // `red` is reused
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t m = wave_shfl_max(mine[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = m;
    }
    __syncthreads();
    if (threadIdx.x < 6) bounds[threadIdx.x] = max(max(red[0][threadIdx.x], red[1][threadIdx.x]), max(red[2][threadIdx.x], red[3][threadIdx.x]));
}
