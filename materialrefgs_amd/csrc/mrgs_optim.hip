// Optimizer step of the training loop: Adam over every parameter tensor in ONE launch.
//
// Replaces torch.optim.Adam(l, lr=0.0, eps=1e-15).step() as set up by GaussianModel.training_setup
// (scene/gaussian_model.py:417-453: ~18 parameter groups with their own learning rates) -- the default single/multi-tensor
// implementation runs 6-8 elementwise passes per tensor (lerp, mul, addcmul, sqrt, div, add, addcdiv), each re-reading its
// operands from HBM.  Here a table of (param, grad, exp_avg, exp_avg_sq, numel, step size, bias correction) rows travels in the
// kernel arguments, workgroup b looks up its tensor with a short scalar scan and every element is read once (16 B) and written
// once (12 B): the kernel is a pure HBM stream, 28 B per element.
//   exp_avg    <- exp_avg + (grad - exp_avg) * (1 - beta1)
//   exp_avg_sq <- exp_avg_sq * beta2 + (1 - beta2) * grad * grad
//   param      <- param - step_size * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps),   step_size = lr / (1 - beta1^t)
// (torch/optim/adam.py _single_tensor_adam, non-capturable, amsgrad = False, weight_decay = 0, maximize = False).
#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_rows_common.h"

namespace {

constexpr int ADAM_MAX = MRGS_ADAM_MAX_TENSORS;
constexpr int ADAM_CHUNK = 4096;                     // elements per workgroup: 256 threads x 4 x float4

struct AdamTable {
    float* p[ADAM_MAX];
    const float* g[ADAM_MAX];
    float* m[ADAM_MAX];
    float* v[ADAM_MAX];
    long long numel[ADAM_MAX];
    unsigned chunk_start[ADAM_MAX + 1];
    float step_size[ADAM_MAX], inv_bc2_sqrt[ADAM_MAX];
    int n;
    float w1, beta2, w2, eps;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float w1, float beta2, float w2, float eps, float step_size,
                                         float inv_bc2_sqrt)
{
    m = fmaf(g - m, w1, m);
    v = fmaf(w2 * g, g, v * beta2);
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

template <bool VEC>
__global__ __launch_bounds__(256) void adam_kernel(AdamTable t)
{
    const unsigned b = blockIdx.x;
    int k = 0;
    while (k + 1 < t.n && b >= t.chunk_start[k + 1]) ++k;             // wave-uniform: scalar loop over <= 32 entries
    const long long n = t.numel[k];
    const long long base = (long long)(b - t.chunk_start[k]) * ADAM_CHUNK;
    float* __restrict__ P = t.p[k];
    const float* __restrict__ G = t.g[k];
    float* __restrict__ M = t.m[k];
    float* __restrict__ V = t.v[k];
    const float ss = t.step_size[k], ib = t.inv_bc2_sqrt[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = base + ((long long)j * 256 + threadIdx.x) * 4;
        if (i >= n) break;
        if (VEC && i + 3 < n) {
            float4 p = *reinterpret_cast<const float4*>(P + i);
            const float4 g = *reinterpret_cast<const float4*>(G + i);
            float4 m = *reinterpret_cast<const float4*>(M + i);
            float4 v = *reinterpret_cast<const float4*>(V + i);
            adam_one(p.x, g.x, m.x, v.x, t.w1, t.beta2, t.w2, t.eps, ss, ib);
            adam_one(p.y, g.y, m.y, v.y, t.w1, t.beta2, t.w2, t.eps, ss, ib);
            adam_one(p.z, g.z, m.z, v.z, t.w1, t.beta2, t.w2, t.eps, ss, ib);
            adam_one(p.w, g.w, m.w, v.w, t.w1, t.beta2, t.w2, t.eps, ss, ib);
            *reinterpret_cast<float4*>(P + i) = p;
            *reinterpret_cast<float4*>(M + i) = m;
            *reinterpret_cast<float4*>(V + i) = v;
        } else {
            for (int e = 0; e < 4 && i + e < n; ++e) {
                float p = P[i + e], m = M[i + e], v = V[i + e];
                adam_one(p, G[i + e], m, v, t.w1, t.beta2, t.w2, t.eps, ss, ib);
                P[i + e] = p; M[i + e] = m; V[i + e] = v;
            }
        }
    }
}

// ---- the rows a view touched only (mrgs_adam_step_rows) ---------------------------------------------------------------------------
// A view touches about half of the surfels; the gradient rows of the others are exact zeros, and the dense
// step still streams them and still moves them by their decaying momentum.  Here rows whose mask byte is 0 keep their bits.
//   * Work is dealt as in adam_kernel: workgroup b owns ADAM_CHUNK consecutive ELEMENTS of one tensor, thread t of pass j the
//     16-byte piece at element base + (j 256 + t) 4.  Lanes walk elements, not rows, so a wave's 64 pieces are 1 KiB contiguous
//     whatever the row width.  A piece has exactly one owner: no atomics, no races -- also where a row boundary or a chunk boundary
//     falls inside a row (widths 3, 45, 160), because ownership never looks at rows.
//   * The rows of a chunk are first_row .. first_row + ceil(4096 / w): at most 4097 mask bytes.  The workgroup ORs the (up to four)
//     masks over that range into LDS once, a 32-bit word per load where the masks are 4-byte aligned and the word lies inside
//     [0, n_rows), single bytes at the ragged end or for unaligned masks; every later mask test is an LDS byte read.
//   * element -> row: first_row = base / w once per workgroup on wave-uniform values (a 64-bit multiply-high with the table's
//     floor(2^63 / w) + 1, exact below 2^43 elements for w <= 2^20), then (offset in the chunk) / w per piece with the table's
//     floor(2^32 / w) + 1, exact while (w + 4096) w < 2^32, i.e. for every w <= MRGS_ADAM_ROWS_MAX_WIDTH.  No runtime division.
//   * A piece inside ONE row (the common case for wide rows) tests one byte; invisible, it issues no load and no store.  A piece over
//     several rows tests each element; with no visible element it is skipped as well, otherwise it is loaded whole, the visible
//     elements go through adam_one, the others keep the loaded bits, and the piece is stored whole.
//   * A tensor that is not 16-byte aligned (its bit of vec_bits clear; decided per tensor, not per launch as in adam_kernel) and the
//     last, short piece of a tensor take the scalar path: visible elements only.
constexpr int ROWS_LDS_WORDS = (ADAM_CHUNK + 3) / 4 + 2;    // rows first_row & ~3 .. first_row + 4096, in words of four

struct AdamRowsTable {
    AdamTable a;
    unsigned w[ADAM_MAX], magic32[ADAM_MAX];
    unsigned long long magic63[ADAM_MAX];
    const uint8_t* mask[MRGS_ADAM_ROWS_MAX_MASKS];
    long long n_rows;
    int n_masks, mask_words;
    unsigned vec_bits;                  // bit k: the four pointers of tensor k are 16-byte aligned
};

__device__ __forceinline__ unsigned rows_div(unsigned q, unsigned w, unsigned magic32) { return w == 1 ? q : __umulhi(q, magic32); }

__global__ __launch_bounds__(256) void adam_rows_kernel(AdamRowsTable t)
{
    __shared__ unsigned s_vis32[ROWS_LDS_WORDS];
    const unsigned b = blockIdx.x;
    int k = 0;
    while (k + 1 < t.a.n && b >= t.a.chunk_start[k + 1]) ++k;         // wave-uniform: scalar loop over <= 32 entries
    const long long n = t.a.numel[k];
    const long long base = (long long)(b - t.a.chunk_start[k]) * ADAM_CHUNK;
    const unsigned w = t.w[k], magic = t.magic32[k];
    // first_row = floor(base / w): the 128-bit product base * magic63 shifted right by 63
    const unsigned long long mg = t.magic63[k], ub = (unsigned long long)base;
    const long long first_row = (long long)((__umul64hi(ub, mg) << 1) | ((ub * mg) >> 63));
    const unsigned off = (unsigned)(base - first_row * (long long)w);          // 0 .. w - 1: where in its row the chunk begins
    const unsigned cnt = (unsigned)(n - base < ADAM_CHUNK ? n - base : ADAM_CHUNK);
    const long long row0 = first_row & ~3ll;                                   // the row of LDS byte 0
    const unsigned lds0 = (unsigned)(first_row - row0);
    const unsigned n_words = ((lds0 + rows_div(off + cnt - 1, w, magic)) >> 2) + 1;     // <= (3 + 4096) / 4 + 1

    for (unsigned wi = threadIdx.x; wi < n_words; wi += 256) {
        const long long r = row0 + 4ll * wi;
        unsigned word = 0;
        if (t.mask_words && r + 3 < t.n_rows) {
            for (int q = 0; q < t.n_masks; ++q) word |= *reinterpret_cast<const unsigned*>(t.mask[q] + r);
        } else {
            for (int e = 0; e < 4 && r + e < t.n_rows; ++e)
                for (int q = 0; q < t.n_masks; ++q) word |= (unsigned)t.mask[q][r + e] << (8 * e);
        }
        s_vis32[wi] = word;
    }
    __syncthreads();
    const uint8_t* s_vis = reinterpret_cast<const uint8_t*>(s_vis32) + lds0;   // s_vis[r] != 0: row first_row + r is visible

    float* __restrict__ P = t.a.p[k];
    const float* __restrict__ G = t.a.g[k];
    float* __restrict__ M = t.a.m[k];
    float* __restrict__ V = t.a.v[k];
    const float ss = t.a.step_size[k], ib = t.a.inv_bc2_sqrt[k];
    const float w1 = t.a.w1, beta2 = t.a.beta2, w2 = t.a.w2, eps = t.a.eps;
    const bool vec = (t.vec_bits >> k) & 1u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned e0 = ((unsigned)j * 256 + threadIdx.x) * 4;             // the piece's first element, counted from base
        if (e0 >= cnt) break;
        const unsigned len = cnt - e0 < 4 ? cnt - e0 : 4;
        const unsigned ra = rows_div(off + e0, w, magic), rb = rows_div(off + e0 + len - 1, w, magic);
        unsigned vis;                                                          // bit e: element e0 + e lies in a visible row
        if (ra == rb) vis = s_vis[ra] ? 15u : 0u;
        else {
            vis = 0;
            for (unsigned e = 0; e < len; ++e) vis |= (s_vis[rows_div(off + e0 + e, w, magic)] ? 1u : 0u) << e;
        }
        if (vis == 0) continue;
        const long long i = base + e0;
        if (vec && len == 4) {
            float4 p = *reinterpret_cast<const float4*>(P + i);
            const float4 g = *reinterpret_cast<const float4*>(G + i);
            float4 m = *reinterpret_cast<const float4*>(M + i);
            float4 v = *reinterpret_cast<const float4*>(V + i);
            if (vis & 1u) adam_one(p.x, g.x, m.x, v.x, w1, beta2, w2, eps, ss, ib);
            if (vis & 2u) adam_one(p.y, g.y, m.y, v.y, w1, beta2, w2, eps, ss, ib);
            if (vis & 4u) adam_one(p.z, g.z, m.z, v.z, w1, beta2, w2, eps, ss, ib);
            if (vis & 8u) adam_one(p.w, g.w, m.w, v.w, w1, beta2, w2, eps, ss, ib);
            *reinterpret_cast<float4*>(P + i) = p;
            *reinterpret_cast<float4*>(M + i) = m;
            *reinterpret_cast<float4*>(V + i) = v;
        } else {
            for (unsigned e = 0; e < len; ++e) {
                if (!((vis >> e) & 1u)) continue;
                float p = P[i + e], m = M[i + e], v = V[i + e];
                adam_one(p, G[i + e], m, v, w1, beta2, w2, eps, ss, ib);
                P[i + e] = p; M[i + e] = m; V[i + e] = v;
            }
        }
    }
}

// the two scalars of adam_one that depend on a tensor's step count, in the precision torch forms them (python doubles, rounded once)
inline void adam_step_scalars(double lr, int32_t step, double beta1, double beta2, bool bias_correction, float& step_size, float& inv_bc2_sqrt)
{
    if (!bias_correction) { step_size = (float)lr; inv_bc2_sqrt = 1.0f; return; }
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    step_size = (float)(lr / bc1);
    inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
}

}   // namespace

extern "C" int mrgs_adam_step_rows(const MrgsAdamRowsTensor* tensors, int32_t n_tensors, int64_t n_rows, const uint8_t* const* masks,
                                   int32_t n_masks, int32_t bias_correction, double beta1, double beta2, double eps, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && !tensors) || n_rows < 0) return MRGS_E_BAD_ARG;
    if (n_masks < 1 || n_masks > MRGS_ADAM_ROWS_MAX_MASKS || !masks) return MRGS_E_BAD_ARG;
    if (n_rows >= (1ll << 43)) return MRGS_E_UNSUPPORTED;
    bool mask_words = true;
    for (int32_t q = 0; q < n_masks; ++q) {
        if (!masks[q] && n_rows > 0) return MRGS_E_BAD_ARG;
        mask_words = mask_words && (((uintptr_t)masks[q]) & 3) == 0;
    }
    long long window_chunks = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {                           // the whole list before the first launch: a refused call moves nothing
        const MrgsAdamRowsTensor& a = tensors[i];
        if (a.numel < 0 || a.row_floats < 0 || a.step < 1) return MRGS_E_BAD_ARG;
        if (a.row_floats > MRGS_ADAM_ROWS_MAX_WIDTH) return MRGS_E_UNSUPPORTED;
        if (a.numel != n_rows * (int64_t)a.row_floats) return MRGS_E_BAD_ARG;           // < 2^43 * 2^15: no overflow
        if (a.numel >= (1ll << 43)) return MRGS_E_UNSUPPORTED;
        if (a.numel > 0 && (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq)) return MRGS_E_BAD_ARG;
        if (i % ADAM_MAX == 0) window_chunks = 0;                       // the launches below take ADAM_MAX list entries each
        window_chunks += (a.numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (window_chunks > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    bool launched = false;
    for (int32_t first = 0; first < n_tensors; first += ADAM_MAX) {
        AdamRowsTable t;
        AdamTable& d = t.a;
        d.n = 0;
        d.w1 = (float)(1.0 - beta1); d.beta2 = (float)beta2; d.w2 = (float)(1.0 - beta2); d.eps = (float)eps;      // as mrgs_adam_step
        unsigned chunks = 0;
        t.vec_bits = 0;
        for (int32_t i = first; i < n_tensors && i < first + ADAM_MAX; ++i) {
            const MrgsAdamRowsTensor& a = tensors[i];
            if (a.numel == 0) continue;
            const long long nch = (a.numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
            const int k = d.n++;
            d.p[k] = a.param; d.g[k] = a.grad; d.m[k] = a.exp_avg; d.v[k] = a.exp_avg_sq; d.numel[k] = a.numel;
            d.chunk_start[k] = chunks;
            chunks += (unsigned)nch;
            adam_step_scalars((double)a.lr, a.step, beta1, beta2, bias_correction != 0, d.step_size[k], d.inv_bc2_sqrt[k]);
            const unsigned w = (unsigned)a.row_floats;
            t.w[k] = w;
            t.magic32[k] = w == 1 ? 0u : (unsigned)((1ull << 32) / w + 1);
            t.magic63[k] = (1ull << 63) / w + 1;
            if ((((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) & 15) == 0) t.vec_bits |= 1u << k;
        }
        if (d.n == 0) continue;
        d.chunk_start[d.n] = chunks;
        for (int q = 0; q < MRGS_ADAM_ROWS_MAX_MASKS; ++q) t.mask[q] = q < n_masks ? masks[q] : nullptr;
        t.n_rows = n_rows; t.n_masks = n_masks; t.mask_words = mask_words ? 1 : 0;
        adam_rows_kernel<<<dim3(chunks), 256, 0, st>>>(t);
        launched = true;
    }
    return launched ? MRGS_LAUNCH_STATUS() : MRGS_OK;              // (an empty model is no HIP call at all)
}

extern "C" int mrgs_adam_step(const MrgsAdamTensor* tensors, int32_t n_tensors, double beta1, double beta2, double eps, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t first = 0; first < n_tensors; first += ADAM_MAX) {
        AdamTable t;
        t.n = 0;
        // the scalars of the update in the precision torch applies them: python doubles rounded to fp32 at the tensor op
        // (1 - beta) must be formed in double: 1 - (float)0.999 is off by 1.3e-5 relative
        t.w1 = (float)(1.0 - beta1); t.beta2 = (float)beta2; t.w2 = (float)(1.0 - beta2); t.eps = (float)eps;
        unsigned chunks = 0;
        bool vec = true;
        for (int32_t i = first; i < n_tensors && i < first + ADAM_MAX; ++i) {
            const MrgsAdamTensor& a = tensors[i];
            if (a.numel < 0 || a.step < 1) return MRGS_E_BAD_ARG;
            if (a.numel == 0) continue;
            if (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq) return MRGS_E_BAD_ARG;
            const long long nch = (a.numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
            if (nch + chunks > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
            const int k = t.n++;
            t.p[k] = a.param; t.g[k] = a.grad; t.m[k] = a.exp_avg; t.v[k] = a.exp_avg_sq; t.numel[k] = a.numel;
            t.chunk_start[k] = chunks;
            chunks += (unsigned)nch;
            adam_step_scalars((double)a.lr, a.step, beta1, beta2, true, t.step_size[k], t.inv_bc2_sqrt[k]);
            vec = vec && ((((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq) & 15) == 0);
        }
        if (t.n == 0) continue;
        t.chunk_start[t.n] = chunks;
        if (vec) adam_kernel<true><<<dim3(chunks), 256, 0, st>>>(t);
        else adam_kernel<false><<<dim3(chunks), 256, 0, st>>>(t);
    }
    return MRGS_LAUNCH_STATUS();
}

// ---- densify / prune compaction (scene/gaussian_model.py:856-905: _prune_optimizer + prune_points) -------------------------------
// The reference drops pruned gaussians with `tensor[mask]` on each of ~16 parameter tensors, their two Adam moments and three
// statistics vectors: ~50 boolean-index calls, each with its own nonzero() pass and host sync.  Here the keep mask is scanned once
// (count per 1024-row block, then one workgroup scans the block counts: block_counts_exclusive_scan, mrgs_wave.h) and ONE launch
// gathers the surviving rows of every tensor: grid = (row blocks, tensors), rows keep their order (stable, like boolean indexing).
// The tensor list is validated whole before the first launch and chunked into launch tables by tensor_table_chunks (mrgs_rows_common.h).
namespace {

constexpr int COMPACT_ROWS = 1024;      // rows per workgroup

struct CompactTable {
    const float* src[MRGS_COMPACT_MAX_TENSORS];
    float* dst[MRGS_COMPACT_MAX_TENSORS];
    int row_floats[MRGS_COMPACT_MAX_TENSORS];
};

__global__ __launch_bounds__(256) void compact_count_kernel(long long n, const uint8_t* __restrict__ keep, unsigned* __restrict__ block_count)
{
    __shared__ unsigned s_wave[4];
    const long long r0 = (long long)blockIdx.x * COMPACT_ROWS + threadIdx.x * 4;
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += (r0 + j < n && keep[r0 + j]) ? 1u : 0u;
    unsigned total;
    block_exclusive_scan_256(c, s_wave, total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void compact_scan_kernel(int nblocks, const unsigned* __restrict__ block_count, unsigned* __restrict__ block_off,
                                                            long long* __restrict__ total_out)
{
    __shared__ unsigned s_wave[16];
    const unsigned total = block_counts_exclusive_scan<1024>(nblocks, block_count, block_off, s_wave);
    if (threadIdx.x == 0) total_out[0] = (long long)total;
}

__global__ __launch_bounds__(256) void compact_gather_kernel(long long n, const uint8_t* __restrict__ keep, const unsigned* __restrict__ block_off,
                                                             CompactTable t)
{
    __shared__ unsigned s_wave[4];
    __shared__ unsigned s_dst[COMPACT_ROWS];        // destination row of each kept row of this block, 0xFFFFFFFF for dropped rows
    const long long rb = (long long)blockIdx.x * COMPACT_ROWS, r0 = rb + threadIdx.x * 4;
    unsigned k[4], c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { k[j] = (r0 + j < n && keep[r0 + j]) ? 1u : 0u; c += k[j]; }
    unsigned total;
    unsigned pre = block_exclusive_scan_256(c, s_wave, total) + block_off[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) { s_dst[threadIdx.x * 4 + j] = k[j] ? pre : 0xFFFFFFFFu; pre += k[j]; }
    __syncthreads();
    if (total == 0) return;
    const int ti = blockIdx.y, L = t.row_floats[ti];
    const float* __restrict__ src = t.src[ti] + rb * L;
    float* __restrict__ dst = t.dst[ti];
    const long long rows = n - rb < COMPACT_ROWS ? n - rb : COMPACT_ROWS;
    const int ne = (int)rows * L;
    for (int e = threadIdx.x; e < ne; e += 256) {
        const int row = e / L, col = e - row * L;
        const unsigned d = s_dst[row];
        if (d != 0xFFFFFFFFu) dst[(size_t)d * L + col] = src[e];
    }
}

}   // namespace

extern "C" size_t mrgs_compact_ws_bytes(int64_t n_rows)
{
    if (n_rows <= 0) return 256;
    const size_t nb = (size_t)((n_rows + COMPACT_ROWS - 1) / COMPACT_ROWS);
    return mrgs_align_up(2 * nb * sizeof(unsigned), 256) + 256;
}

extern "C" int mrgs_compact_count(int64_t n_rows, const uint8_t* keep, void* ws, size_t ws_bytes, int64_t* count_dev, void* stream)
{
    if (n_rows < 0 || !ws || !count_dev || ws_bytes < mrgs_compact_ws_bytes(n_rows)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) { MRGS_HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st)); return MRGS_OK; }
    if (!keep) return MRGS_E_BAD_ARG;
    const long long nb = (n_rows + COMPACT_ROWS - 1) / COMPACT_ROWS;
    if (nb > (1 << 22)) return MRGS_E_UNSUPPORTED;
    unsigned* counts = (unsigned*)ws;
    unsigned* offs = counts + nb;
    compact_count_kernel<<<dim3((unsigned)nb), 256, 0, st>>>(n_rows, keep, counts);
    compact_scan_kernel<<<1, 1024, 0, st>>>((int)nb, counts, offs, (long long*)count_dev);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_compact_rows(int64_t n_rows, const uint8_t* keep, const void* ws, const MrgsCompactTensor* tensors, int32_t n_tensors,
                                 void* stream)
{
    if (n_rows < 0 || n_tensors < 0 || (n_tensors > 0 && !tensors)) return MRGS_E_BAD_ARG;
    if (n_rows == 0 || n_tensors == 0) return MRGS_OK;
    if (!keep || !ws) return MRGS_E_BAD_ARG;
    const long long nb = (n_rows + COMPACT_ROWS - 1) / COMPACT_ROWS;
    const unsigned* offs = (const unsigned*)ws + nb;
    for (int32_t i = 0; i < n_tensors; ++i) {                           // the whole list before the first launch: a refused call moves nothing
        const MrgsCompactTensor& e = tensors[i];
        if (e.row_floats < 0 || e.row_floats > (1 << 20)) return MRGS_E_BAD_ARG;
        if (e.row_floats != 0 && (!e.src || !e.dst)) return MRGS_E_BAD_ARG;
    }
    tensor_table_chunks<CompactTable>(
        tensors, n_tensors,
        [](CompactTable& t, int m, const MrgsCompactTensor& e) { t.src[m] = e.src; t.dst[m] = e.dst; t.row_floats[m] = e.row_floats; },
        [&](const CompactTable& t, int m) {
            compact_gather_kernel<<<dim3((unsigned)nb, (unsigned)m), 256, 0, (hipStream_t)stream>>>(n_rows, keep, offs, t);
        });
    return MRGS_LAUNCH_STATUS();
}
