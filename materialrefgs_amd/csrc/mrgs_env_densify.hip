// EnvGaussianModel.densify_and_prune and add_densification_stats (scene/env_gaussian_model.py:384-603; contract in include/mrgs.h).
//
// The reference runs six data-dependent torch stages -- clone, split in 2, opacity prune, quantile-of-weights prune with split in 5,
// top-k visibility cap, reset -- and re-materialises every parameter tensor, both Adam moments and four statistics vectors up to eight
// times on the way.  Everything those stages decide follows per SOURCE row from seven numbers (accum, denom, max_radii2D, weight_accum,
// two raw scalings, raw opacity), three global maxima (W0, W1, W4) and two order statistics (the 0.1 quantile q, the visibility cut).
// A source row yields at most two "slot rows" after stage 2 -- {original, clone} or {child 0, child 1}; slot sigma = 0 original, 1 clone,
// 2 + k stage-2 child k -- and each slot row ends as nothing, one row or five stage-4 children: ten "entries" a row, e = 5 a + j.
// The final order is segment-major over 24 segments (kept slot sigma: segment sigma; stage-4 child j of slot sigma: 4 + 4 j + sigma),
// rows ascending inside a segment: exactly the order the reference's cats and boolean prunes leave.
//   reduce passes   grid-stride over rows, 28 B read per row each, every one re-deriving the row's state from the seven numbers instead
//                   of storing it: W0 = max w; W1 = max(W0, clone weights) with the stage-1/2 counts; the stage-3 survivors' wavg (8 B
//                   written per row) and their count n; after the quantile the stage-4 states (a 4-byte record per row), W4 and the
//                   counts; the ten entry keys of stage 5 (40 B written per row).
//   select          radix select over the order-preserving integer image of the float, 8-bit digits from the top: per pass one histogram
//                   launch (bins in LDS, one global add per non-empty bin and block) and one one-block launch that picks the digit.
//                   Exact k-th smallest, the count below it and the count equal to it; no sort.
//   rank passes     one thread per row, 256 rows per block, ranks inside a block from wave ballots, 24 segment counts per block written
//                   to a [24][blocks] matrix and scanned segment-major by one block (one block_counts_exclusive_scan, mrgs_wave.h, over all 24 rows): first the rows equal to the cut (the tie rule is
//                   "earlier row goes first"), then the survivors (the destinations).  The host reads the totals once.
//   emit            grid (row blocks, tensors): a block rebuilds its rows' up to ten destinations in LDS from the records and streams
//                   its slab of one source once.  Per tensor of L floats a row: reads 4 L P bytes, writes 4 L bytes per output row.
// The weight path and the radius path are single IEEE fp32 operations (the file is built without contraction): bit-equal to the fp32
// torch restatement.  NaN in weight_accum is not served (fmax semantics, where torch's max() would propagate it).
#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_philox.h"
#include "mrgs_rows_common.h"

namespace {

constexpr int ROWS = 256;                       // rows per workgroup of the rank and emit passes, one per thread
constexpr int NSEG = 24, NENT = 10;
constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr unsigned ABSENT = 0x7FFFFFFFu;        // float bits of an entry that does not exist: its key is the largest of all
constexpr int REDUCE_BLOCKS = 256;              // grid of the reduce passes: bounds the same-address atomics of a launch
constexpr float DIV2 = 1.6f, DIV4 = 2.5f;       // 0.8 * 2 and 0.5 * 5
constexpr float RATIO2 = 0.625f;                // fl32(1 / 1.6); the stage-4 ratio fl32(1 / 2.5) only scales values that are reset

// device scalars (uint32 words)
enum { S_W0, S_W1, S_W4, S_Q, S_N3, S_N4, S_NCLONE, S_NSPLIT2, S_PRUNE4, S_SPLIT4, S_PRUNE5, S_F, S_HI, S_MINABOVE, S_WORDS = 16 };
struct SelState { unsigned active, prefix, k, k0, less, equal, pad0, pad1; };
constexpr size_t SEL_BYTES = sizeof(SelState) + 4 * 256 * sizeof(unsigned);
constexpr size_t HEAD_BYTES = 8192;             // scalars | select state | four histograms, cleared per call

__device__ __forceinline__ unsigned sel_key(unsigned bits)           // -0 and +0 are one value
{
    if ((bits << 1) == 0u) bits = 0u;
    return ord_f(__uint_as_float(bits));
}

struct EnvArgs {
    long long P, n_after;
    float max_grad, min_opacity, dense_limit, world_limit, screen_limit;
    int has_screen;
    const float *accum, *denom, *radii, *weight, *scaling, *opacity;
};

struct Row {
    bool split2, clone, faint;
    bool present[2];
    float weight[2], wavg[2], rad[2], m[2], d;
};

__device__ __forceinline__ float nan_to_zero(float v) { return v != v ? 0.0f : v; }

// stages 1-3 of one source row
__device__ __forceinline__ Row row_eval(const EnvArgs& a, long long i, float W0, float W1)
{
    Row r;
    const float d = a.denom[i], w = a.weight[i], rad = a.radii[i];
    const float g = nan_to_zero(__fdiv_rn(a.accum[i], d));
    const float s0 = expf(a.scaling[2 * i]), s1 = expf(a.scaling[2 * i + 1]), ms = fmaxf(s0, s1);
    const float o = 1.0f / (1.0f + expf(-a.opacity[i]));
    r.d = d;
    r.clone = fabsf(g) >= a.max_grad && ms <= a.dense_limit;
    r.split2 = g >= a.max_grad && ms > a.dense_limit;
    r.faint = o < a.min_opacity;
    if (r.split2) {
        const float mc = fmaxf(expf(logf(s0 / DIV2)), expf(logf(s1 / DIV2)));     // exp of the raw value the emit pass writes
        r.present[0] = r.present[1] = !r.faint;
        r.weight[0] = r.weight[1] = w * W1;
        r.rad[0] = r.rad[1] = rad * RATIO2;
        r.m[0] = r.m[1] = mc;
    } else {
        r.present[0] = !r.faint; r.present[1] = r.clone && !r.faint;
        r.weight[0] = w; r.weight[1] = w * W0;
        r.rad[0] = r.rad[1] = rad;
        r.m[0] = r.m[1] = ms;
    }
    r.wavg[0] = nan_to_zero(__fdiv_rn(r.weight[0], d));
    r.wavg[1] = nan_to_zero(__fdiv_rn(r.weight[1], d));
    return r;
}

// stage 4 of one slot row: 0 gone, 1 kept, 2 replaced by five children
__device__ __forceinline__ unsigned stage4_state(const EnvArgs& a, const Row& r, int s, float q)
{
    if (!r.present[s]) return 0u;
    const bool big = (a.has_screen && r.rad[s] > a.screen_limit) || r.m[s] > a.world_limit;
    if (!big) return 1u;
    return r.wavg[s] < q ? 0u : 2u;
}

__device__ __forceinline__ void block_add(unsigned v, unsigned* dst)
{
    v = wave_shfl_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}
__device__ __forceinline__ void block_max(unsigned v, unsigned* dst)
{
    v = wave_shfl_max(v);
    if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, v);
}

// ---- reduce passes ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void env_w0_kernel(long long P, const float* __restrict__ w, unsigned* __restrict__ scal)
{
    unsigned best = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) best = max(best, ord_f(w[i]));
    block_max(best, scal + S_W0);
}

__global__ __launch_bounds__(256) void env_w1_kernel(EnvArgs a, unsigned* __restrict__ scal)
{
    const float W0 = unord_f(scal[S_W0]);
    unsigned best = scal[S_W0], nc = 0, ns = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += (long long)gridDim.x * 256) {
        const Row r = row_eval(a, i, W0, 0.0f);
        if (r.clone) { best = max(best, ord_f(r.weight[1])); ++nc; }              // the clone is appended whether or not stage 3 removes it
        if (r.split2) ++ns;
    }
    block_max(best, scal + S_W1);
    block_add(nc, scal + S_NCLONE);
    block_add(ns, scal + S_NSPLIT2);
}

__global__ __launch_bounds__(256) void env_keys4_kernel(EnvArgs a, unsigned* __restrict__ scal, unsigned* __restrict__ keys)
{
    const float W0 = unord_f(scal[S_W0]), W1 = unord_f(scal[S_W1]);
    unsigned n = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += (long long)gridDim.x * 256) {
        const Row r = row_eval(a, i, W0, W1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            keys[(size_t)s * a.P + i] = r.present[s] ? __float_as_uint(r.wavg[s]) : ABSENT;
            n += r.present[s];
        }
    }
    block_add(n, scal + S_N3);
}

__global__ __launch_bounds__(256) void env_stage4_kernel(EnvArgs a, unsigned* __restrict__ scal, unsigned* __restrict__ rec)
{
    const float W0 = unord_f(scal[S_W0]), W1 = unord_f(scal[S_W1]), q = __uint_as_float(scal[S_Q]);
    unsigned best = 0, n4 = 0, np = 0, ns = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += (long long)gridDim.x * 256) {
        const Row r = row_eval(a, i, W0, W1);
        unsigned word = r.split2 ? 1u : 0u;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned st = stage4_state(a, r, s, q);
            word |= st << (1 + 2 * s);
            if (st) best = max(best, ord_f(r.weight[s]));                         // rows left after this stage's prune, the split sources included
            n4 += st == 1u ? 1u : st == 2u ? 5u : 0u;
            np += r.present[s] && st == 0u;
            ns += st == 2u;
        }
        rec[i] = word;
    }
    block_max(best, scal + S_W4);
    block_add(n4, scal + S_N4);
    block_add(np, scal + S_PRUNE4);
    block_add(ns, scal + S_SPLIT4);
}

__global__ __launch_bounds__(256) void env_keys5_kernel(EnvArgs a, const unsigned* __restrict__ scal, const unsigned* __restrict__ rec,
                                                        unsigned* __restrict__ keys)
{
    const float W0 = unord_f(scal[S_W0]), W1 = unord_f(scal[S_W1]), W4 = unord_f(scal[S_W4]);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += (long long)gridDim.x * 256) {
        const Row r = row_eval(a, i, W0, W1);
        const unsigned word = rec[i];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned st = (word >> (1 + 2 * s)) & 3u;
            const unsigned kept = __float_as_uint(r.wavg[s]);
            const unsigned child = __float_as_uint(nan_to_zero(__fdiv_rn(r.weight[s] * W4, r.d)));
#pragma unroll
            for (int j = 0; j < 5; ++j)
                keys[(size_t)(5 * s + j) * a.P + i] = st == 2u ? child : (st == 1u && j == 0) ? kept : ABSENT;
        }
    }
}

// ---- radix select ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sel_hist_kernel(const unsigned* __restrict__ vals, long long M, const SelState* __restrict__ st,
                                                       unsigned* __restrict__ hist, int pass)
{
    __shared__ unsigned h[256];
    if (!st->active) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u, prefix = st->prefix;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) {
        const unsigned key = sel_key(vals[i]);
        if ((key & himask) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(hist + pass * 256 + threadIdx.x, h[threadIdx.x]);
}

__global__ __launch_bounds__(256) void sel_pick_kernel(SelState* __restrict__ st, const unsigned* __restrict__ hist, int pass)
{
    __shared__ unsigned s_wave[4];
    if (!st->active) return;
    const unsigned c = hist[pass * 256 + threadIdx.x], k = st->k;
    unsigned total;
    const unsigned before = block_exclusive_scan_256(c, s_wave, total);
    if (k >= before && k < before + c) {                                          // exactly one thread (k < total)
        st->prefix |= threadIdx.x << (24 - 8 * pass);
        st->k = k - before;
        if (pass == 3) { st->less = st->k0 - (k - before); st->equal = c; }
    }
}

__global__ void sel_set_kernel(SelState* st, unsigned k)
{
    st->active = 1u; st->prefix = 0u; st->k = st->k0 = k;
}
__global__ void sel_out_kernel(const SelState* st, unsigned* out)
{
    out[0] = __float_as_uint(unord_f(st->prefix)); out[1] = st->less; out[2] = st->equal; out[3] = st->k0;
}

// smallest key above the selected one (the next order statistic when the selected value occurs no further)
__global__ __launch_bounds__(256) void sel_above_kernel(const unsigned* __restrict__ vals, long long M, const SelState* __restrict__ st,
                                                        unsigned* __restrict__ scal)
{
    if (!st->active) return;
    const unsigned cut = st->prefix;
    unsigned best = 0xFFFFFFFFu;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) {
        const unsigned key = sel_key(vals[i]);
        if (key > cut) best = min(best, key);
    }
    best = ~wave_shfl_max(~best);
    if ((threadIdx.x & 63) == 0 && best != 0xFFFFFFFFu) atomicMin(scal + S_MINABOVE, best);
}

// rank = 0.1f (n - 1): which order statistics the quantile needs
__global__ void env_quantile_setup_kernel(unsigned* scal, SelState* st)
{
    const unsigned n = scal[S_N3];
    scal[S_MINABOVE] = 0xFFFFFFFFu;
    st->prefix = 0u;
    if (n == 0u) { st->active = 0u; return; }
    const float rank = __fmul_rn(0.1f, (float)(n - 1u)), lo = floorf(rank), hi = ceilf(rank);
    scal[S_F] = __float_as_uint(__fsub_rn(rank, lo));
    scal[S_HI] = (unsigned)hi;
    st->active = 1u; st->k = st->k0 = (unsigned)lo;
}

__global__ void env_quantile_kernel(unsigned* scal, const SelState* st)
{
    if (!st->active) { scal[S_Q] = 0u; return; }
    const float v_lo = unord_f(st->prefix);
    const float v_hi = scal[S_HI] < st->less + st->equal ? v_lo : unord_f(scal[S_MINABOVE]);
    const float f = __uint_as_float(scal[S_F]), diff = __fsub_rn(v_hi, v_lo);
    const float q = f < 0.5f ? __fadd_rn(v_lo, __fmul_rn(f, diff)) : __fsub_rn(v_hi, __fmul_rn(diff, __fsub_rn(1.0f, f)));
    scal[S_Q] = __float_as_uint(q);
}

// stage 5: how many rows go, and the rank of the last of them
__global__ void env_cap_setup_kernel(unsigned* scal, SelState* st, unsigned* hist, long long n_after)
{
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x) return;
    const long long total = scal[S_N4], n_prune = total - n_after;
    st->prefix = 0u; st->less = 0u; st->equal = 0u;
    if (n_prune <= 0 || total == 0) { st->active = 0u; scal[S_PRUNE5] = 0u; return; }
    const unsigned np = (unsigned)(n_prune < total ? n_prune : total);
    scal[S_PRUNE5] = np;
    st->active = 1u; st->k = st->k0 = np - 1u;
}

// ---- rank passes -----------------------------------------------------------------------------------------------------------------
// segment of entry e of a row whose record is `word`
__device__ __forceinline__ int entry_segment(unsigned word, int s, int j, bool child) { const int sigma = 2 * (int)(word & 1u) + s; return child ? 4 + 4 * j + sigma : sigma; }

// flags: bit seg set when this thread's row has an entry in the segment (at most one).  rank[seg]: rows of the block before this one with the
// bit set; s_tot[seg][wave] the wave totals.  One barrier.
__device__ __forceinline__ void segment_ranks(unsigned flags, unsigned (&rank)[NSEG], unsigned (*s_tot)[4])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned in_wave[NSEG];
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
        const unsigned long long b = __ballot((flags >> s) & 1u);
        in_wave[s] = (unsigned)__popcll(b & below);
        if (lane == 0) s_tot[s][wave] = (unsigned)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NSEG; ++s) {
        unsigned base = 0;
        for (int w = 0; w < wave; ++w) base += s_tot[s][w];
        rank[s] = base + in_wave[s];
    }
}

__device__ __forceinline__ void write_block_counts(unsigned (*s_tot)[4], unsigned* __restrict__ mat, int nblocks)
{
    if (threadIdx.x < NSEG) mat[(size_t)threadIdx.x * nblocks + blockIdx.x] = s_tot[threadIdx.x][0] + s_tot[threadIdx.x][1] + s_tot[threadIdx.x][2] + s_tot[threadIdx.x][3];
}

// entries of a row that exist after stage 4 (stage == 0) or survive stage 5 (stage == 1), as a 10-bit mask over e = 5 s + j
__device__ __forceinline__ unsigned entry_mask(unsigned word, int stage)
{
    unsigned m = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const unsigned st = (word >> (1 + 2 * s)) & 3u;
        unsigned e = st == 2u ? 31u : st == 1u ? 1u : 0u;
        if (stage) e &= (word >> (8 + 5 * s)) & 31u;
        m |= e << (5 * s);
    }
    return m;
}
__device__ __forceinline__ unsigned segment_flags(unsigned word, unsigned emask)
{
    unsigned flags = 0;
#pragma unroll
    for (int e = 0; e < NENT; ++e)
        if ((emask >> e) & 1u) flags |= 1u << entry_segment(word, e / 5, e % 5, ((word >> (1 + 2 * (e / 5))) & 3u) == 2u);
    return flags;
}

// rows equal to the cut, per segment and block
__global__ __launch_bounds__(256) void env_ties_kernel(long long P, int nblocks, const unsigned* __restrict__ rec, const unsigned* __restrict__ keys,
                                                       const SelState* __restrict__ st, unsigned* __restrict__ mat)
{
    __shared__ unsigned s_tot[NSEG][4];
    const long long i = (long long)blockIdx.x * ROWS + threadIdx.x;
    const unsigned word = i < P ? rec[i] : 0u;
    unsigned ties = 0;
    if (st->active) {
        const unsigned emask = entry_mask(word, 0), cut = st->prefix;
#pragma unroll
        for (int e = 0; e < NENT; ++e)
            if (((emask >> e) & 1u) && sel_key(keys[(size_t)e * P + i]) == cut) ties |= 1u << e;
    }
    unsigned rank[NSEG];
    segment_ranks(segment_flags(word, ties), rank, s_tot);
    write_block_counts(s_tot, mat, nblocks);
}

// stage 5's verdict into the record, survivors per segment and block
__global__ __launch_bounds__(256) void env_final_kernel(long long P, int nblocks, unsigned* __restrict__ rec, const unsigned* __restrict__ keys,
                                                        const SelState* __restrict__ st, const unsigned* __restrict__ scal,
                                                        const unsigned* __restrict__ tie_off, unsigned* __restrict__ mat)
{
    __shared__ unsigned s_tot[NSEG][4], s_tot2[NSEG][4];
    const long long i = (long long)blockIdx.x * ROWS + threadIdx.x;
    unsigned word = i < P ? rec[i] : 0u;
    const unsigned emask = entry_mask(word, 0);
    unsigned survive = emask;
    if (st->active) {                                                             // uniform
        const unsigned cut = st->prefix, ties_go = scal[S_PRUNE5] - st->less;
        unsigned ties = 0, below = 0;
#pragma unroll
        for (int e = 0; e < NENT; ++e)
            if ((emask >> e) & 1u) {
                const unsigned key = sel_key(keys[(size_t)e * P + i]);
                ties |= (unsigned)(key == cut) << e;
                below |= (unsigned)(key < cut) << e;
            }
        unsigned rank[NSEG];
        segment_ranks(segment_flags(word, ties), rank, s_tot);
        survive &= ~below;
#pragma unroll
        for (int e = 0; e < NENT; ++e)
            if ((ties >> e) & 1u) {
                const int seg = entry_segment(word, e / 5, e % 5, ((word >> (1 + 2 * (e / 5))) & 3u) == 2u);
                if (tie_off[(size_t)seg * nblocks + blockIdx.x] + rank[seg] < ties_go) survive &= ~(1u << e);
            }
    }
    word = (word & 0xFFu) | ((survive & 31u) << 8) | (((survive >> 5) & 31u) << 13);
    if (i < P) rec[i] = word;
    unsigned rank2[NSEG];
    segment_ranks(segment_flags(word, survive), rank2, s_tot2);
    write_block_counts(s_tot2, mat, nblocks);
}

// exclusive scan of mat [NSEG][nblocks] in segment-major order; with counts: the 24 segment totals, their sum and the call's figures
__global__ __launch_bounds__(1024) void env_scan_kernel(int nblocks, const unsigned* __restrict__ mat, unsigned* __restrict__ off,
                                                        const unsigned* __restrict__ scal, const SelState* __restrict__ st, long long* __restrict__ counts)
{
    __shared__ unsigned s_wave[16];
    const unsigned grand = block_counts_exclusive_scan<1024>(NSEG * nblocks, mat, off, s_wave);
    if (!counts) return;
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < NSEG) {
        const unsigned lo = off[(size_t)threadIdx.x * nblocks];
        const unsigned hi = threadIdx.x == NSEG - 1 ? grand : off[(size_t)(threadIdx.x + 1) * nblocks];
        counts[threadIdx.x] = (long long)(hi - lo);
    }
    if (threadIdx.x == 0) {
        counts[24] = grand;
        counts[25] = scal[S_NCLONE]; counts[26] = scal[S_NSPLIT2]; counts[27] = scal[S_N3]; counts[28] = scal[S_PRUNE4];
        counts[29] = scal[S_SPLIT4]; counts[30] = scal[S_PRUNE5]; counts[31] = scal[S_Q];
        counts[32] = __float_as_uint(unord_f(scal[S_W0])); counts[33] = __float_as_uint(unord_f(scal[S_W1]));
        counts[34] = __float_as_uint(unord_f(scal[S_W4])); counts[35] = st->active ? __float_as_uint(unord_f(st->prefix)) : 0u;
        counts[36] = scal[S_N4]; counts[37] = st->active; counts[38] = 0; counts[39] = 0;
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------
struct EmitArgs {
    long long P, n_rows;
    int nblocks;
    const float *xyz, *scaling, *rotation, *noise, *noise4;
    unsigned long long seed;
};

// coordinate `col` of the centre of slot sigma of source row `row` (j < 0) or of its stage-4 child j: each generation adds
// R(normalize(q)) (s_x z0, s_y z1, 0) with the scale of the row it splits (env_gaussian_model.py:413-418, 435-441)
__device__ __forceinline__ float entry_centre(const EmitArgs& a, long long row, int sigma, int j, int col)
{
    const RotationRow2 R = rotation_row2(a.rotation + 4 * (size_t)row, col);
    float s0 = expf(a.scaling[2 * (size_t)row]), s1 = expf(a.scaling[2 * (size_t)row + 1]);
    float c = a.xyz[3 * (size_t)row + col], z0, z1;
    if (sigma >= 2) {
        const int k = sigma - 2;
        if (a.noise) { const float* n = a.noise + ((size_t)row * 2 + k) * 2; z0 = n[0]; z1 = n[1]; }
        else normal_pair(a.seed, row, k, z0, z1);
        c = c + (R.R0 * (s0 * z0) + R.R1 * (s1 * z1));
        s0 = expf(logf(s0 / DIV2)); s1 = expf(logf(s1 / DIV2));
    }
    if (j >= 0) {
        if (a.noise4) { const float* n = a.noise4 + (((size_t)row * 4 + sigma) * 5 + j) * 2; z0 = n[0]; z1 = n[1]; }
        else normal_pair(a.seed, row, j, z0, z1, 1u + (unsigned)sigma);
        c = c + (R.R0 * (s0 * z0) + R.R1 * (s1 * z1));
    }
    return c;
}

__global__ __launch_bounds__(256) void env_emit_kernel(EmitArgs a, const unsigned* __restrict__ rec, const unsigned* __restrict__ off, EmitTable t)
{
    __shared__ unsigned s_tot[NSEG][4];
    __shared__ unsigned s_dst[NENT][ROWS];          // destination row of each entry (valid where the record's mask has the bit)
    __shared__ unsigned s_word[ROWS];
    const long long rb = (long long)blockIdx.x * ROWS, i = rb + threadIdx.x;
    const unsigned word = i < a.P ? rec[i] : 0u;
    const unsigned emask = entry_mask(word, 1);
    unsigned rank[NSEG];
    segment_ranks(segment_flags(word, emask), rank, s_tot);
#pragma unroll
    for (int e = 0; e < NENT; ++e) {
        unsigned d = NONE;
        if ((emask >> e) & 1u) {
            const int seg = entry_segment(word, e / 5, e % 5, ((word >> (1 + 2 * (e / 5))) & 3u) == 2u);
            d = off[(size_t)seg * a.nblocks + blockIdx.x] + rank[seg];
            if (d >= a.n_rows) d = NONE;                                          // cannot happen with the counts this workspace produced
        }
        s_dst[e][threadIdx.x] = d;
    }
    s_word[threadIdx.x] = word;
    __syncthreads();
    const int ti = blockIdx.y, L = t.row_floats[ti], role = t.role[ti];
    const float* __restrict__ src = t.src[ti] + (size_t)rb * L;
    float* __restrict__ dst = t.dst[ti];
    const long long rows = a.P - rb < ROWS ? a.P - rb : ROWS;
    const int ne = (int)rows * L;
    for (int el = threadIdx.x; el < ne; el += 256) {
        const int row = el / L, col = el - row * L;
        const unsigned w = s_word[row];
        unsigned m = entry_mask(w, 1);
        if (!m) continue;
        const float v = src[el];
        const int split2 = (int)(w & 1u);
        const float v1 = role == MRGS_DENSIFY_SCALING && split2 ? logf(expf(v) / DIV2) : v;       // the value of the slot row itself
        const float v2 = role == MRGS_DENSIFY_SCALING ? logf(expf(v1) / DIV4) : v1;               // ... of its stage-4 children
        while (m) {
            const int e = __ffs(m) - 1;
            m &= m - 1u;
            const unsigned d = s_dst[e][row];
            if (d == NONE) continue;
            const int s = e / 5, j = e - 5 * s, sigma = 2 * split2 + s;
            const bool child = ((w >> (1 + 2 * s)) & 3u) == 2u;
            float out = child ? v2 : v1;
            if (role == MRGS_DENSIFY_MOMENT) out = (sigma == 0 && !child) ? v : 0.0f;
            else if (role == MRGS_DENSIFY_XYZ && (child || sigma >= 2)) out = entry_centre(a, rb + row, sigma, child ? j : -1, col);
            dst[(size_t)d * L + col] = out;
        }
    }
}

__global__ __launch_bounds__(256) void env_stats_kernel(long long P, const float* __restrict__ grad, const uint8_t* __restrict__ visible,
                                                        const float* __restrict__ weight, float* __restrict__ accum, float* __restrict__ denom,
                                                        float* __restrict__ weight_accum)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !visible[i]) return;
    densify_stats_row(grad, i, accum, denom);
    if (weight) weight_accum[i] += weight[i];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline long long env_blocks(int64_t P) { return (P + ROWS - 1) / ROWS; }
inline int reduce_grid(int64_t n) { const int64_t b = (n + 255) / 256; return (int)(b < REDUCE_BLOCKS ? b : REDUCE_BLOCKS); }

struct EnvWs {
    unsigned* scal; SelState* sel; unsigned* hist; unsigned* keys; unsigned* rec; unsigned* mat; unsigned* off;
    size_t total;
};
EnvWs env_carve(void* base, int64_t P)
{
    EnvWs w;
    uint8_t* p = (uint8_t*)base;
    w.scal = (unsigned*)p; w.sel = (SelState*)(p + 256); w.hist = (unsigned*)(p + 512);
    p += HEAD_BYTES;
    w.keys = (unsigned*)p; p += mrgs_align_up((size_t)NENT * P * 4, 256);
    w.rec = (unsigned*)p; p += mrgs_align_up((size_t)P * 4, 256);
    const size_t m = mrgs_align_up((size_t)NSEG * env_blocks(P) * 4, 256);
    w.mat = (unsigned*)p; p += m;
    w.off = (unsigned*)p; p += m;
    w.total = (size_t)(p - (uint8_t*)base);
    return w;
}

void launch_select(const unsigned* vals, long long M, SelState* st, unsigned* hist, hipStream_t s)
{
    for (int pass = 0; pass < 4; ++pass) {
        sel_hist_kernel<<<reduce_grid(M) * 4, 256, 0, s>>>(vals, M, st, hist, pass);
        sel_pick_kernel<<<1, 256, 0, s>>>(st, hist, pass);
    }
}

int env_check_cfg(const MrgsEnvDensifyConfig* cfg)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsEnvDensifyConfig)) return MRGS_E_BAD_ARG;
    if (cfg->P < 0 || cfg->n_after < 0 || !(cfg->max_grad > 0.0f) || (cfg->flags & ~3u)) return MRGS_E_BAD_ARG;
    if (cfg->flags & MRGS_ENV_DENSIFY_SPLIT_SCREEN) return MRGS_E_UNSUPPORTED;
    if (cfg->P * (int64_t)NENT >= (1ll << 31)) return MRGS_E_UNSUPPORTED;
    return MRGS_OK;
}

}   // namespace

extern "C" size_t mrgs_env_densify_ws_bytes(int64_t P)
{
    if (P <= 0) return 256;
    return env_carve(nullptr, P).total;
}

extern "C" int mrgs_env_densify_classify(const MrgsEnvDensifyConfig* cfg, const float* accum, const float* denom, const float* max_radii,
                                         const float* weight_accum, const float* scaling_raw, const float* opacity_raw, void* ws, size_t ws_bytes,
                                         int64_t* counts_dev, void* stream)
{
    if (int rc = env_check_cfg(cfg)) return rc;
    if (cfg->P == 0) return MRGS_OK;
    if (!ws || ((uintptr_t)ws & 255) || !counts_dev || ws_bytes < mrgs_env_densify_ws_bytes(cfg->P)) return MRGS_E_BAD_ARG;
    if (!accum || !denom || !max_radii || !weight_accum || !scaling_raw || !opacity_raw) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t P = cfg->P;
    const EnvWs w = env_carve(ws, P);
    EnvArgs a;
    a.P = P; a.n_after = cfg->n_after; a.max_grad = cfg->max_grad; a.min_opacity = cfg->min_opacity; a.dense_limit = cfg->percent_dense_extent;
    a.world_limit = cfg->world_size_limit; a.screen_limit = cfg->max_screen_size; a.has_screen = (cfg->flags & MRGS_ENV_DENSIFY_SCREEN) ? 1 : 0;
    a.accum = accum; a.denom = denom; a.radii = max_radii; a.weight = weight_accum; a.scaling = scaling_raw; a.opacity = opacity_raw;
    const int rg = reduce_grid(P), nb = (int)env_blocks(P);
    MRGS_HIP_TRY(hipMemsetAsync(ws, 0, HEAD_BYTES, st));
    env_w0_kernel<<<rg, 256, 0, st>>>(P, weight_accum, w.scal);
    env_w1_kernel<<<rg, 256, 0, st>>>(a, w.scal);
    env_keys4_kernel<<<rg, 256, 0, st>>>(a, w.scal, w.keys);
    env_quantile_setup_kernel<<<1, 1, 0, st>>>(w.scal, w.sel);
    launch_select(w.keys, 2 * P, w.sel, w.hist, st);
    sel_above_kernel<<<reduce_grid(2 * P), 256, 0, st>>>(w.keys, 2 * P, w.sel, w.scal);
    env_quantile_kernel<<<1, 1, 0, st>>>(w.scal, w.sel);
    env_stage4_kernel<<<rg, 256, 0, st>>>(a, w.scal, w.rec);
    env_keys5_kernel<<<rg, 256, 0, st>>>(a, w.scal, w.rec, w.keys);
    env_cap_setup_kernel<<<1, 256, 0, st>>>(w.scal, w.sel, w.hist, cfg->n_after);
    launch_select(w.keys, (long long)NENT * P, w.sel, w.hist, st);
    env_ties_kernel<<<nb, 256, 0, st>>>(P, nb, w.rec, w.keys, w.sel, w.mat);
    env_scan_kernel<<<1, 1024, 0, st>>>(nb, w.mat, w.off, w.scal, w.sel, nullptr);
    env_final_kernel<<<nb, 256, 0, st>>>(P, nb, w.rec, w.keys, w.sel, w.scal, w.off, w.mat);
    env_scan_kernel<<<1, 1024, 0, st>>>(nb, w.mat, w.off, w.scal, w.sel, (long long*)counts_dev);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_env_densify_emit(const MrgsEnvDensifyConfig* cfg, const void* ws, int64_t n_rows, const MrgsDensifyTensor* tensors,
                                     int32_t n_tensors, uint64_t seed, const float* noise, const float* noise4, void* stream)
{
    if (int rc = env_check_cfg(cfg)) return rc;
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return MRGS_E_BAD_ARG;
    if (cfg->P == 0 || n_tensors == 0) return MRGS_OK;
    if (!ws || ((uintptr_t)ws & 255) || n_rows < 0 || n_rows > (int64_t)NENT * cfg->P) return MRGS_E_BAD_ARG;
    const bool empty = n_rows == 0;                                               // every destination is empty: its pointer may be NULL
    if (int rc = densify_check_tensors(tensors, n_tensors, empty, cfg->xyz_raw, cfg->scaling_raw, cfg->rotation_raw)) return rc;
    if (empty) return MRGS_OK;
    const EnvWs w = env_carve(const_cast<void*>(ws), cfg->P);
    EmitArgs a;
    a.P = cfg->P; a.n_rows = n_rows; a.nblocks = (int)env_blocks(cfg->P);
    a.xyz = cfg->xyz_raw; a.scaling = cfg->scaling_raw; a.rotation = cfg->rotation_raw; a.noise = noise; a.noise4 = noise4; a.seed = seed;
    const bool any = tensor_table_chunks<EmitTable>(tensors, n_tensors, emit_table_fill, [&](const EmitTable& t, int m) {
        env_emit_kernel<<<dim3((unsigned)a.nblocks, (unsigned)m), 256, 0, (hipStream_t)stream>>>(a, w.rec, w.off, t);
    });
    if (!any) return MRGS_OK;                                                     // every tensor has empty rows: nothing was queued
    return MRGS_LAUNCH_STATUS();
}

extern "C" size_t mrgs_env_select_ws_bytes(void) { return mrgs_align_up(SEL_BYTES, 256); }

extern "C" int mrgs_env_select(int64_t n, const float* values, int64_t k, void* ws, size_t ws_bytes, uint32_t* out_dev, void* stream)
{
    if (n < 0 || n >= (1ll << 31) || k < 0 || (n > 0 && k >= n)) return MRGS_E_BAD_ARG;
    if (n == 0) return MRGS_OK;
    if (!values || !ws || ((uintptr_t)ws & 255) || !out_dev || ws_bytes < mrgs_env_select_ws_bytes()) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    SelState* sel = (SelState*)ws;
    unsigned* hist = (unsigned*)((uint8_t*)ws + sizeof(SelState));
    MRGS_HIP_TRY(hipMemsetAsync(ws, 0, SEL_BYTES, st));
    sel_set_kernel<<<1, 1, 0, st>>>(sel, (unsigned)k);
    launch_select((const unsigned*)values, n, sel, hist, st);
    sel_out_kernel<<<1, 1, 0, st>>>(sel, out_dev);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_env_densify_stats(int64_t P, const float* grad, const uint8_t* visible, const float* weight_accumulate, float* accum,
                                      float* denom, float* weight_accum, void* stream)
{
    if (P < 0 || P >= (1ll << 31) * 256) return MRGS_E_BAD_ARG;
    if (P == 0) return MRGS_OK;
    if (!grad || !visible || !accum || !denom || (weight_accumulate && !weight_accum)) return MRGS_E_BAD_ARG;
    env_stats_kernel<<<dim3((unsigned)((P + 255) / 256)), 256, 0, (hipStream_t)stream>>>(P, grad, visible, weight_accumulate, accum, denom, weight_accum);
    return MRGS_LAUNCH_STATUS();
}
