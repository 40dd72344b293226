// Evaluation of one rendered view: the numbers and the 8-bit pictures of eval.py (render_set :23-74, render_set_train :76-102) and of
// evaluate_psnr / training_report (train_refreal.py:1656-1735).
//
// What the reference runs per view after the render -- two clamps, five depthwise 11x11 conv2d launches and ~20 elementwise kernels for SSIM,
// three .item() reads, and per saved map mul / add / clamp / permute / to(uint8) with a blocking copy (torchvision.utils.save_image), the depth
// map through numpy and cv2 (utils/image_utils.py:73-80) -- is here
//   eval_metrics_kernel    one 32x32 tile per workgroup and channel: both images clamped to [0, 1] AS THEY ARE READ (eval.py:44-46; no clamped
//                          copy exists), the window moments by the tile passes of mrgs_ssim_tile.h (the ones loss_fwd_kernel runs), SSIM,
//                          |x - y| and (x - y)^2 reduced per workgroup in a fixed order.  No derivative maps: the workspace is the partials.
//   eval_finalize_kernel   one workgroup sums the partials in double, fixed order, and writes the 8 numbers (both PSNR conventions)
//   export_minmax_kernel   per-workgroup minima / maxima of the DEPTH maps (only launched when there is one)
//   export_rgb8_kernel     up to 16 maps -> uint8 [n_maps, H, W, 3]; a workgroup converts 1024 pixels of one map into LDS bytes and
//                          stores them as aligned dwords with a byte head and tail
// Nothing is read back by the host in either call.
//
// The 8-bit rule is torchvision's x.mul(255).add_(0.5).clamp_(0, 255).to(uint8): the product and the sum are rounded separately, so they
// are written with __fmul_rn / __fadd_rn (the file keeps the default flags, contraction on, like mrgs_loss.hip whose tile passes it shares).
// DEPTH is visualize_depth's fp32 chain in its order; its division is the compiler's correctly rounded one (no fast-math in this build).
#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_ssim_tile.h"
#include "mrgs_rgb8.h"      // the jet table, to_byte, block_minmax, store_lds_bytes: shared with mrgs_sheet.hip

namespace {

// ---- metrics ------------------------------------------------------------------------------------------------------------------------
constexpr int EPART = 4;          // floats per workgroup partial: ssim, l1, sq, 0 (one 16-byte row)

struct EvalArgs {
    int H, W;
    float w[2 * LR + 1];
};

__global__ __launch_bounds__(256) void eval_metrics_kernel(EvalArgs a, const float* __restrict__ img, const float* __restrict__ gt,
                                                            float* __restrict__ partials)
{
    __shared__ float s1[LH][LH + 1], s2[LH][LH + 1];
    __shared__ float hz[5][LH][LT + 1];
    __shared__ float red[4][EPART];
    const int H = a.H, W = a.W, c = blockIdx.z;
    const int bx = blockIdx.x * LT, by = blockIdx.y * LT, tid = threadIdx.x;
    const size_t HW = (size_t)H * W;
    ssim_tile_stage<true>(img + c * HW, gt + c * HW, H, W, bx, by, tid, s1, s2);
    __syncthreads();
    ssim_tile_rows(a.w, tid, s1, s2, hz);
    __syncthreads();
    const int tx = tid & (LT - 1), y0 = (tid / LT) * LP;
    float mom[5][LP];
    ssim_tile_cols(a.w, tx, y0, hz, mom);
    float part[3] = {0.f, 0.f, 0.f};
    const int x = bx + tx;
#pragma unroll
    for (int o = 0; o < LP; ++o) {
        const int y = by + y0 + o;
        if ((x >= W) | (y >= H)) continue;
        const float d = s1[y0 + o + LR][tx + LR] - s2[y0 + o + LR][tx + LR];      // the clamped values
        part[0] += ssim_point(mom[0][o], mom[1][o], mom[2][o], mom[3][o], mom[4][o]).S;
        part[1] += fabsf(d); part[2] += d * d;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) part[k] = wave_shfl_sum(part[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) red[tid >> 6][k] = part[k];
    __syncthreads();
    if (tid < EPART) {
        const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partials[b * EPART + tid] = tid < 3 ? (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]) : 0.f;
    }
}

// out[0] psnr of the whole image, [1] ssim, [2] l1, [3] mean of the per-channel psnr (out_terms[6] of the fused loss), [4..6] mse per
// channel, [7] 0
__global__ __launch_bounds__(256) void eval_finalize_kernel(EvalArgs a, const float* __restrict__ partials, int blocks_per_channel,
                                                             float* __restrict__ out)
{
    __shared__ double red[4][5];
    const int tid = threadIdx.x;
    double acc[5] = {0, 0, 0, 0, 0};                                       // ssim, l1, sq[0..2]
    const int nb = blocks_per_channel * 3;
    for (int b = tid; b < nb; b += 256) {                                  // the order of the additions is fixed
        const float4 p = reinterpret_cast<const float4*>(partials)[b];
        const int ch = b / blocks_per_channel;
        acc[0] += p.x; acc[1] += p.y;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[2 + k] += ch == k ? (double)p.z : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double v = wave_shfl_sum(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double s[5];
        for (int k = 0; k < 5; ++k) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        const double HW = (double)a.H * a.W, N = HW * 3.0;
        float ps = 0.f;
        for (int k = 0; k < 3; ++k) {                                       // utils/image_utils.py:20-23 on [3,H,W]: one mse per channel
            const float mse = (float)(s[2 + k] / HW);
            out[4 + k] = mse;
            ps += 20.f * log10f(1.f / sqrtf(mse));
        }
        const float mse_all = (float)(((s[2] + s[3]) + s[4]) / N);          // ... on [1,3,H,W] (eval.py:51): one mse for the image
        out[0] = 20.f * log10f(1.f / sqrtf(mse_all));                        // mse 0: 1 / 0 = inf, log10(inf) = inf, as the reference
        out[1] = (float)(s[0] / N); out[2] = (float)(s[1] / N); out[3] = ps / 3.f; out[7] = 0.f;
    }
}

// ---- 8-bit export ---------------------------------------------------------------------------------------------------------------------
constexpr int XMM = 256;          // workgroups (= partial rows) per DEPTH map of the min/max launch, at most

struct ExportArgs {
    int n_maps, mm_blocks;
    size_t HW;
    const float* data[MRGS_EXPORT_MAX_MAPS];
    uint8_t channels[MRGS_EXPORT_MAX_MAPS], mode[MRGS_EXPORT_MAX_MAPS], depth_slot[MRGS_EXPORT_MAX_MAPS];
    uint8_t depth_map[MRGS_EXPORT_MAX_MAPS];      // depth_map[slot] = index of the map
};

// minimum and maximum of every DEPTH map, NaN skipped (fminf / fmaxf); exact in any order.  grid (mm_blocks, n_depth)
__global__ __launch_bounds__(256) void export_minmax_kernel(ExportArgs a, float2* __restrict__ partials)
{
    __shared__ float red[4][2];
    const int tid = threadIdx.x, slot = blockIdx.y;
    const float* __restrict__ d = a.data[a.depth_map[slot]];
    float mn = INFINITY, mx = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < a.HW; i += (size_t)gridDim.x * 256) {
        const float v = d[i];
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    const float2 r = block_minmax(mn, mx, tid, red);
    if (tid == 0) partials[(size_t)slot * XMM + blockIdx.x] = r;
}

// grid (ceil(HW / XCHUNK), n_maps).  The chunk's 3 n bytes start at global byte `obase` of `out`; LDS holds them shifted by obase & 3, so
// that a 4-byte aligned global address is a 4-byte aligned LDS offset and the body goes out as whole dwords.
__global__ __launch_bounds__(256) void export_rgb8_kernel(ExportArgs a, const float2* __restrict__ partials, uint8_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[3 * XCHUNK + 8];
    __shared__ float red[4][2];
    const int tid = threadIdx.x, k = blockIdx.y;
    const int mode = a.mode[k], C = a.channels[k];
    const size_t HW = a.HW, p0 = (size_t)blockIdx.x * XCHUNK;
    const int n = (int)(HW - p0 < (size_t)XCHUNK ? HW - p0 : (size_t)XCHUNK);     // pixels of this chunk, >= 1
    const size_t obase = ((size_t)k * HW + p0) * 3;
    const int shift = (int)(obase & 3);
    float mn = 0.f, den = 1.f;
    if (mode == MRGS_EXPORT_DEPTH) {            // wave-uniform: the map's minimum and maximum from the first launch's partial rows
        float lo = INFINITY, hi = -INFINITY;
        if (tid < a.mm_blocks) { const float2 p = partials[(size_t)a.depth_slot[k] * XMM + tid]; lo = p.x; hi = p.y; }
        const float2 r = block_minmax(lo, hi, tid, red);
        mn = r.x;
        const float mx = r.y;
        den = __fsub_rn(__fadd_rn(1e-20f, mx), mn);                                // 1e-20 + depth.max() - depth.min()
    }
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ src = a.data[k] + (size_t)c * HW + p0;
        float v[4];
        const bool vec = (n == XCHUNK) & ((reinterpret_cast<uintptr_t>(src) & 15) == 0);   // uniform: a whole chunk at a 16-byte aligned address
        if (vec) {
            const float4 f = reinterpret_cast<const float4*>(src)[tid];
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int i = tid + 256 * j; v[j] = i < n ? src[i] : 0.f; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = vec ? 4 * tid + j : tid + 256 * j;
            if (i >= n) continue;
            float x = v[j];
            if (mode == MRGS_EXPORT_DEPTH) {
                // (depth - min) / (1e-20 + max - min), then (depth * 255).clip(0, 255).astype(uint8): image_utils.py:75-76
                const uint32_t level = to_byte(__fmul_rn(__fsub_rn(x, mn) / den, 255.f));
                sb[shift + 3 * i] = d_jet.rgb[level][0]; sb[shift + 3 * i + 1] = d_jet.rgb[level][1]; sb[shift + 3 * i + 2] = d_jet.rgb[level][2];
                continue;
            }
            if (mode == MRGS_EXPORT_NORMAL) x = __fadd_rn(__fmul_rn(x, 0.5f), 0.5f);      // eval.py:56
            const uint8_t b = (uint8_t)to_byte(__fadd_rn(__fmul_rn(x, 255.f), 0.5f));
            if (C == 1) { sb[shift + 3 * i] = b; sb[shift + 3 * i + 1] = b; sb[shift + 3 * i + 2] = b; }   // repeat(3, 1, 1), eval.py:63-64
            else sb[shift + 3 * i + c] = b;
        }
    }
    __syncthreads();
    store_lds_bytes(sb, shift, 3 * n, out, obase, tid);
}

}   // namespace

extern "C" size_t mrgs_eval_metrics_ws_bytes(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return 0;
    return (size_t)((W + LT - 1) / LT) * ((H + LT - 1) / LT) * 3 * EPART * sizeof(float);
}

extern "C" int mrgs_eval_metrics(const MrgsEvalConfig* cfg, const float* image, const float* gt, void* ws, size_t ws_bytes, float* out,
                                 void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsEvalConfig) || cfg->H <= 0 || cfg->W <= 0 || cfg->flags != 0) return MRGS_E_BAD_ARG;
    if (!image || !gt || !ws || !out || (reinterpret_cast<uintptr_t>(ws) & 15)) return MRGS_E_BAD_ARG;
    if (ws_bytes < mrgs_eval_metrics_ws_bytes(cfg->H, cfg->W)) return MRGS_E_WORKSPACE;
    EvalArgs a;
    a.H = cfg->H; a.W = cfg->W;
    ssim_window(a.w);
    const dim3 grid((a.W + LT - 1) / LT, (a.H + LT - 1) / LT, 3);
    if (grid.y > 65535u || (size_t)grid.x * grid.y * 3 > 0x7fffffffu) return MRGS_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    eval_metrics_kernel<<<grid, 256, 0, st>>>(a, image, gt, (float*)ws);
    eval_finalize_kernel<<<1, 256, 0, st>>>(a, (const float*)ws, (int)(grid.x * grid.y), out);
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}

extern "C" size_t mrgs_export_ws_bytes(void) { return (size_t)MRGS_EXPORT_MAX_MAPS * XMM * sizeof(float2); }

extern "C" int mrgs_eval_jet_table(uint8_t* table768)
{
    if (!table768) return MRGS_E_BAD_ARG;
    for (int L = 0; L < 256; ++L)
        for (int c = 0; c < 3; ++c) table768[3 * L + c] = JET.rgb[L][c];
    return MRGS_OK;
}

extern "C" int mrgs_export_rgb8(const MrgsExportConfig* cfg, const MrgsExportMap* maps, void* ws, size_t ws_bytes, uint8_t* out, void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsExportConfig) || cfg->H <= 0 || cfg->W <= 0 || cfg->flags != 0) return MRGS_E_BAD_ARG;
    if (cfg->n_maps < 1 || cfg->n_maps > MRGS_EXPORT_MAX_MAPS || !maps || !out || (reinterpret_cast<uintptr_t>(out) & 3)) return MRGS_E_BAD_ARG;
    ExportArgs a = {};
    a.n_maps = cfg->n_maps;
    a.HW = (size_t)cfg->H * cfg->W;
    int n_depth = 0;
    for (int k = 0; k < cfg->n_maps; ++k) {
        const MrgsExportMap& m = maps[k];
        if (!m.data || (reinterpret_cast<uintptr_t>(m.data) & 3) || (m.channels != 1 && m.channels != 3)) return MRGS_E_BAD_ARG;
        if (m.mode != MRGS_EXPORT_UNIT && m.mode != MRGS_EXPORT_NORMAL && m.mode != MRGS_EXPORT_DEPTH) return MRGS_E_BAD_ARG;
        if (m.mode == MRGS_EXPORT_DEPTH && m.channels != 1) return MRGS_E_BAD_ARG;
        a.data[k] = m.data; a.channels[k] = (uint8_t)m.channels; a.mode[k] = (uint8_t)m.mode;
        if (m.mode == MRGS_EXPORT_DEPTH) { a.depth_slot[k] = (uint8_t)n_depth; a.depth_map[n_depth++] = (uint8_t)k; }
    }
    const size_t chunks = (a.HW + XCHUNK - 1) / XCHUNK;
    if (chunks > 0x7fffffffu) return MRGS_E_UNSUPPORTED;
    if (n_depth && (!ws || (reinterpret_cast<uintptr_t>(ws) & 7))) return MRGS_E_BAD_ARG;
    if (n_depth && ws_bytes < mrgs_export_ws_bytes()) return MRGS_E_WORKSPACE;
    a.mm_blocks = (int)(chunks < (size_t)XMM ? chunks : (size_t)XMM);
    hipStream_t st = (hipStream_t)stream;
    if (n_depth) export_minmax_kernel<<<dim3(a.mm_blocks, n_depth), 256, 0, st>>>(a, (float2*)ws);
    export_rgb8_kernel<<<dim3((unsigned)chunks, cfg->n_maps), 256, 0, st>>>(a, (const float2*)ws, out);
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}
