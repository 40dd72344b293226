// densify_and_prune and the densification statistics (scene/gaussian_model.py:975-1061; contract in include/mrgs.h).
//
// The reference runs three torch stages -- clone + cat, split + cat + prune, final prune -- that materialise a P + |C| and a
// P + |C| + N |S| copy of every parameter tensor and both Adam moments on the way (~50 boolean-index calls with a nonzero() and a
// host sync each, 16 repeat()s and 16 cat()s twice over).  Everything those stages decide follows per SOURCE row from five numbers
// (accum, denom, two raw scalings, raw opacity), so here they are two passes:
//   classify  one thread per row, 1024 rows per workgroup: a class byte per row (bit 0 keep the original, bit 1 emit a clone, bit 2
//             emit N children), per-block counts of the three output segments, then one workgroup scans each segment's counts
//             (block_counts_exclusive_scan, mrgs_wave.h; offsets restart at 0 per segment) into per-block offsets and
//             the three totals the host reads (24 bytes: the call's only synchronisation).  Reads 20 B, writes 1 B per row.
//   emit      grid (row blocks, tensors): a block rebuilds its rows' three destinations in LDS from the class bytes and the block
//             offsets and streams its slab of one source once; originals, clones and the N children are written from that one read.
//             Per tensor of L floats a row: reads 4 L P bytes, writes 4 L (n_keep + n_clone + N n_child) bytes.
// The split offsets come from a counter-based generator (Philox4x32-10, Salmon et al., SC'11) keyed by the seed with counter
// (source row, child): no state, no dependence on the grid, nothing drawn for rows that are not split.
//   stats     one thread per row, in place: 17 B read and up to 12 B written per visible row, 1 B per invisible one.
#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_philox.h"
#include "mrgs_rows_common.h"

namespace {

constexpr int DENSIFY_ROWS = 1024;              // rows per workgroup (256 threads x 4), as in the compaction of mrgs_optim.hip
constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr unsigned CLS_KEEP = 1u, CLS_CLONE = 2u, CLS_CHILD = 4u;

// the three per-thread counts of a class byte travel through one scan (pack_fields, mrgs_wave.h)
__device__ __forceinline__ unsigned long long pack_counts(unsigned cls) { return pack_fields(cls & 1u, (cls >> 1) & 1u, (cls >> 2) & 1u); }

struct ClassifyArgs {
    long long P;
    float max_grad, min_opacity, dense_limit, world_limit, child_div;
};

__device__ __forceinline__ unsigned classify_row(const ClassifyArgs& a, float accum, float denom, float sc0, float sc1, float op)
{
    float g = __fdiv_rn(accum, denom);                                  // IEEE: a decision input
    if (g != g) g = 0.0f;                                               // never seen: 0 / 0
    const float s0 = expf(sc0), s1 = expf(sc1), ms = fmaxf(s0, s1);
    const float o = 1.0f / (1.0f + expf(-op));
    const bool clone = fabsf(g) >= a.max_grad && ms <= a.dense_limit;
    const bool split = g >= a.max_grad && ms > a.dense_limit;
    const bool faint = o < a.min_opacity;
    const bool gone = faint || (a.world_limit > 0.0f && ms > a.world_limit);
    unsigned cls = 0;
    if (!split && !gone) cls |= CLS_KEEP;
    if (clone && !gone) cls |= CLS_CLONE;
    if (split) {
        // the final prune sees the child's own scale: exp of the raw value the emit pass writes
        const float mc = fmaxf(expf(logf(s0 / a.child_div)), expf(logf(s1 / a.child_div)));
        if (!(faint || (a.world_limit > 0.0f && mc > a.world_limit))) cls |= CLS_CHILD;
    }
    return cls;
}

__global__ __launch_bounds__(256) void densify_classify_kernel(ClassifyArgs a, const float* __restrict__ accum, const float* __restrict__ denom,
                                                               const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                               uint8_t* __restrict__ cls_out, unsigned* __restrict__ block_count, int nblocks)
{
    __shared__ unsigned long long s_wave[4];
    const long long r0 = (long long)blockIdx.x * DENSIFY_ROWS + threadIdx.x * 4;
    unsigned word = 0;
    unsigned long long c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long r = r0 + j;
        if (r < a.P) {
            const unsigned cls = classify_row(a, accum[r], denom[r], scaling[2 * r], scaling[2 * r + 1], opacity[r]);
            word |= cls << (8 * j);
            c += pack_counts(cls);
        }
    }
    *reinterpret_cast<unsigned*>(cls_out + r0) = word;                  // the class array is padded to whole blocks
    unsigned long long total;
    block_exclusive_scan_256(c, s_wave, total);
    if (threadIdx.x < 3) block_count[(size_t)threadIdx.x * nblocks + blockIdx.x] = unpack_field(total, threadIdx.x);
}

// block_count / block_off: [3][nblocks] (originals, clones, children per k); totals: device int64[3]
__global__ __launch_bounds__(1024) void densify_scan_kernel(int nblocks, const unsigned* __restrict__ block_count, unsigned* __restrict__ block_off,
                                                            long long* __restrict__ totals)
{
    __shared__ unsigned s_wave[16];
    for (int seg = 0; seg < 3; ++seg) {                                 // offsets restart per segment: the emit pass adds n_keep and n_keep + n_clone
        const unsigned total = block_counts_exclusive_scan<1024>(nblocks, block_count + (size_t)seg * nblocks, block_off + (size_t)seg * nblocks, s_wave);
        if (threadIdx.x == 0) totals[seg] = (long long)total;
    }
}

struct EmitArgs {
    long long P;
    int N, nblocks;
    unsigned n_keep, n_clone, n_child;
    float child_div;
    const float* xyz;
    const float* scaling;
    const float* rotation;
    const float* noise;
    unsigned long long seed;
};

// coordinate `col` of child k of source row `row`: xyz + R(normalize(q)) (s_x z0, s_y z1, 0)   (gaussian_model.py:984-989, build_rotation)
__device__ __forceinline__ float child_centre(const EmitArgs& a, long long row, int k, int col)
{
    float z0, z1;
    if (a.noise) { const float* z = a.noise + ((size_t)row * a.N + k) * 2; z0 = z[0]; z1 = z[1]; }
    else normal_pair(a.seed, row, k, z0, z1);
    const RotationRow2 R = rotation_row2(a.rotation + 4 * (size_t)row, col);
    const float sx = expf(a.scaling[2 * (size_t)row]) * z0, sy = expf(a.scaling[2 * (size_t)row + 1]) * z1;
    return a.xyz[3 * (size_t)row + col] + (R.R0 * sx + R.R1 * sy);
}

__global__ __launch_bounds__(256) void densify_emit_kernel(EmitArgs a, const uint8_t* __restrict__ cls_in, const unsigned* __restrict__ block_off,
                                                           EmitTable t)
{
    __shared__ unsigned long long s_wave[4];
    __shared__ unsigned s_dst[3][DENSIFY_ROWS];     // destination row of each row's original / clone / first child, NONE when not emitted
    const long long rb = (long long)blockIdx.x * DENSIFY_ROWS;
    const unsigned word = *reinterpret_cast<const unsigned*>(cls_in + rb + threadIdx.x * 4);
    unsigned long long c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += pack_counts((word >> (8 * j)) & 0xFFu);
    unsigned long long total;
    const unsigned long long pre = block_exclusive_scan_256(c, s_wave, total);
    unsigned d[3];
    d[0] = block_off[blockIdx.x] + unpack_field(pre, 0);
    d[1] = a.n_keep + block_off[(size_t)a.nblocks + blockIdx.x] + unpack_field(pre, 1);
    d[2] = a.n_keep + a.n_clone + block_off[2 * (size_t)a.nblocks + blockIdx.x] + unpack_field(pre, 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned cls = (word >> (8 * j)) & 0xFFu;
#pragma unroll
        for (int seg = 0; seg < 3; ++seg) {
            const unsigned on = (cls >> seg) & 1u;
            s_dst[seg][threadIdx.x * 4 + j] = on ? d[seg] : NONE;
            d[seg] += on;
        }
    }
    __syncthreads();
    if (total == 0) return;
    const int ti = blockIdx.y, L = t.row_floats[ti], role = t.role[ti];
    const float* __restrict__ src = t.src[ti] + (size_t)rb * L;
    float* __restrict__ dst = t.dst[ti];
    const long long rows = a.P - rb < DENSIFY_ROWS ? a.P - rb : DENSIFY_ROWS;
    const int ne = (int)rows * L;
    for (int e = threadIdx.x; e < ne; e += 256) {
        const int row = e / L, col = e - row * L;
        const unsigned dk = s_dst[0][row], dc = s_dst[1][row], dh = s_dst[2][row];
        if ((dk & dc & dh) == NONE) continue;
        const float v = src[e];
        if (dk != NONE) dst[(size_t)dk * L + col] = v;
        if (dc != NONE) dst[(size_t)dc * L + col] = role == MRGS_DENSIFY_MOMENT ? 0.0f : v;
        if (dh != NONE) {
            float out = v;
            if (role == MRGS_DENSIFY_MOMENT) out = 0.0f;
            else if (role == MRGS_DENSIFY_SCALING) out = logf(expf(v) / a.child_div);
            for (int k = 0; k < a.N; ++k) {
                if (role == MRGS_DENSIFY_XYZ) out = child_centre(a, rb + row, k, col);
                dst[((size_t)dh + (size_t)k * a.n_child) * L + col] = out;
            }
        }
    }
}

__global__ __launch_bounds__(256) void densify_stats_kernel(long long P, const float* __restrict__ grad, const uint8_t* __restrict__ visible,
                                                            const int* __restrict__ radii, float* __restrict__ accum, float* __restrict__ denom,
                                                            float* __restrict__ max_radii)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !visible[i]) return;
    densify_stats_row(grad, i, accum, denom);
    if (radii && max_radii) max_radii[i] = fmaxf(max_radii[i], (float)radii[i]);
}

inline long long densify_blocks(int64_t P) { return (P + DENSIFY_ROWS - 1) / DENSIFY_ROWS; }
inline size_t densify_cls_bytes(int64_t P) { return mrgs_align_up((size_t)densify_blocks(P) * DENSIFY_ROWS, 256); }

int densify_check_cfg(const MrgsDensifyConfig* cfg)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsDensifyConfig)) return MRGS_E_BAD_ARG;
    if (cfg->P < 0 || cfg->N < 1 || cfg->N > 8 || !(cfg->max_grad > 0.0f)) return MRGS_E_BAD_ARG;
    if (cfg->P * (int64_t)(cfg->N > 2 ? cfg->N : 2) >= (1ll << 31)) return MRGS_E_UNSUPPORTED;
    return MRGS_OK;
}

}   // namespace

extern "C" size_t mrgs_densify_ws_bytes(int64_t P)
{
    if (P <= 0) return 256;
    return densify_cls_bytes(P) + mrgs_align_up(6 * (size_t)densify_blocks(P) * sizeof(unsigned), 256) + 256;
}

extern "C" int mrgs_densify_classify(const MrgsDensifyConfig* cfg, const float* accum, const float* denom, const float* scaling_raw,
                                     const float* opacity_raw, void* ws, size_t ws_bytes, int64_t* counts_dev, void* stream)
{
    if (int rc = densify_check_cfg(cfg)) return rc;
    if (cfg->P == 0) return MRGS_OK;
    if (!ws || ((uintptr_t)ws & 3) || !counts_dev || ws_bytes < mrgs_densify_ws_bytes(cfg->P)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (!accum || !denom || !scaling_raw || !opacity_raw) return MRGS_E_BAD_ARG;
    const long long nb = densify_blocks(cfg->P);
    uint8_t* cls = (uint8_t*)ws;
    unsigned* counts = (unsigned*)(cls + densify_cls_bytes(cfg->P));
    unsigned* offs = counts + 3 * nb;
    ClassifyArgs a;
    a.P = cfg->P; a.max_grad = cfg->max_grad; a.min_opacity = cfg->min_opacity; a.dense_limit = cfg->percent_dense_extent;
    a.world_limit = cfg->world_size_limit; a.child_div = (float)(0.8 * (double)cfg->N);
    densify_classify_kernel<<<dim3((unsigned)nb), 256, 0, st>>>(a, accum, denom, scaling_raw, opacity_raw, cls, counts, (int)nb);
    densify_scan_kernel<<<1, 1024, 0, st>>>((int)nb, counts, offs, (long long*)counts_dev);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_densify_emit(const MrgsDensifyConfig* cfg, const void* ws, const int64_t* counts_host, const MrgsDensifyTensor* tensors,
                                 int32_t n_tensors, uint64_t seed, const float* noise, void* stream)
{
    if (int rc = densify_check_cfg(cfg)) return rc;
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return MRGS_E_BAD_ARG;
    if (cfg->P == 0 || n_tensors == 0) return MRGS_OK;
    if (!ws || ((uintptr_t)ws & 3) || !counts_host) return MRGS_E_BAD_ARG;
    const int64_t n_keep = counts_host[0], n_clone = counts_host[1], n_child = counts_host[2];
    if (n_keep < 0 || n_clone < 0 || n_child < 0 || n_keep > cfg->P || n_clone > cfg->P || n_child > cfg->P) return MRGS_E_BAD_ARG;
    const bool empty = n_keep + n_clone + n_child == 0;                  // every destination is empty: its pointer may be NULL
    if (int rc = densify_check_tensors(tensors, n_tensors, empty, cfg->xyz_raw, cfg->scaling_raw, cfg->rotation_raw)) return rc;
    if (empty) return MRGS_OK;
    const long long nb = densify_blocks(cfg->P);
    const uint8_t* cls = (const uint8_t*)ws;
    const unsigned* offs = (const unsigned*)(cls + densify_cls_bytes(cfg->P)) + 3 * nb;
    EmitArgs a;
    a.P = cfg->P; a.N = cfg->N; a.nblocks = (int)nb;
    a.n_keep = (unsigned)n_keep; a.n_clone = (unsigned)n_clone; a.n_child = (unsigned)n_child;
    a.child_div = (float)(0.8 * (double)cfg->N);
    a.xyz = cfg->xyz_raw; a.scaling = cfg->scaling_raw; a.rotation = cfg->rotation_raw; a.noise = noise; a.seed = seed;
    tensor_table_chunks<EmitTable>(tensors, n_tensors, emit_table_fill, [&](const EmitTable& t, int m) {
        densify_emit_kernel<<<dim3((unsigned)nb, (unsigned)m), 256, 0, (hipStream_t)stream>>>(a, cls, offs, t);
    });
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_densify_stats(int64_t P, const float* grad, const uint8_t* visible, const int32_t* radii, float* accum, float* denom,
                                  float* max_radii, void* stream)
{
    if (P < 0 || P >= (1ll << 31) * 256) return MRGS_E_BAD_ARG;
    if (P == 0) return MRGS_OK;
    if (!grad || !visible || !accum || !denom) return MRGS_E_BAD_ARG;
    densify_stats_kernel<<<dim3((unsigned)((P + 255) / 256)), 256, 0, (hipStream_t)stream>>>(P, grad, visible, radii, accum, denom, max_radii);
    return MRGS_LAUNCH_STATUS();
}
