// The dataset side of a view: what the reference does to a photograph between the file and the loss, on 8-bit planes that stay on the device.
//
//   image_resize_h_kernel / image_resize_v_kernel / image_gather_kernel
//                          PILtoTorch's `pil_image.resize(resolution)` (utils/general_utils.py:21-27): Pillow's BICUBIC on 8-bit channels,
//                          bit for bit.  Pillow runs a horizontal pass into an 8-bit intermediate and then a vertical one, each
//                          clip8((2^21 + sum kk * pixel) >> 22) with integer coefficients kk; the coefficient tables are made on the host in
//                          double (materialrefgs_amd/viewstore.py: resize_table) and arrive as device arrays.  One thread per output byte.
//                          Horizontal: the lanes of a wave walk neighbouring source windows of one row, so a tap step reads one or a few
//                          cache lines that the next steps read again.  Vertical: consecutive lanes are consecutive x, every tap step is one
//                          coalesced row segment and the coefficient is the same for the whole row.
//   image_composite_kernel readCamerasFromTransforms' alpha compositing onto a constant background (scene/dataset_readers.py:276-282), whose
//                          float64 expression and wrapping cast to a byte depend on (colour, alpha) only: a 64 KiB table made by the host
//                          with that literal expression, looked up here.  RGBA pixels in, three byte planes out.
//   view_decode_kernel     one launch per fetched view: byte planes -> the fp32 tensors the losses read (u8 / 255 by IEEE division as torch's
//                          uint8_tensor / 255.0, the grey image with every product and sum rounded separately, the normal prior through a
//                          256-entry table, the mask and the ref-score thresholds).  Four pixels per thread, 16-byte stores where the
//                          planes' offsets allow them.
// Built with -ffp-contract=off (Makefile: FLAGS_mrgs_image): the one floating-point chain, the grey image, must round every product and
// sum on its own, and __fmul_rn / __fadd_rn are plain operators to this compiler, which contraction would fuse into fma.
// No atomics, nothing is read back, nothing is allocated.
#include "mrgs_internal.h"

namespace {

constexpr int PRECISION_BITS = 22;        // Pillow: 32 - 8 - 2

__device__ __forceinline__ uint8_t clip8(int32_t v)
{
    v >>= PRECISION_BITS;                 // arithmetic
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct ResizeArgs {
    int C, rows, in_len, out_len, ksize;  // rows: the extent of the axis that is not resized in this pass
    int64_t sc, sy, sx;                   // source strides in bytes: plane, row, pixel
};

// dst [C][rows][out_len] planar.  bounds [out_len][2] = (first source index, tap count), kk [out_len][ksize]
__global__ __launch_bounds__(256) void image_resize_h_kernel(ResizeArgs a, const uint8_t* __restrict__ src, const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ kk, uint8_t* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.C * a.rows * a.out_len;
    if (i >= total) return;
    const int xx = (int)(i % a.out_len);
    const size_t cy = i / a.out_len;
    const int y = (int)(cy % a.rows), c = (int)(cy / a.rows);
    const int x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
    const uint8_t* __restrict__ p = src + c * a.sc + y * a.sy + x0 * a.sx;
    const int32_t* __restrict__ k = kk + (size_t)xx * a.ksize;
    int32_t acc = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) acc += k[t] * (int32_t)p[t * a.sx];
    dst[i] = clip8(acc);
}

// dst [C][out_len][rows] planar: `rows` is the width here, out_len the new height
__global__ __launch_bounds__(256) void image_resize_v_kernel(ResizeArgs a, const uint8_t* __restrict__ src, const int32_t* __restrict__ bounds,
                                                             const int32_t* __restrict__ kk, uint8_t* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.C * a.rows * a.out_len;
    if (i >= total) return;
    const int x = (int)(i % a.rows);
    const size_t cy = i / a.rows;
    const int yy = (int)(cy % a.out_len), c = (int)(cy / a.out_len);
    const int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
    const uint8_t* __restrict__ p = src + c * a.sc + y0 * a.sy + x * a.sx;
    const int32_t* __restrict__ k = kk + (size_t)yy * a.ksize;
    int32_t acc = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) acc += k[t] * (int32_t)p[t * a.sy];
    dst[i] = clip8(acc);
}

// equal sizes: strided source -> planar copy.  rows = H, out_len = W
__global__ __launch_bounds__(256) void image_gather_kernel(ResizeArgs a, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.C * a.rows * a.out_len;
    if (i >= total) return;
    const int x = (int)(i % a.out_len);
    const size_t cy = i / a.out_len;
    const int y = (int)(cy % a.rows), c = (int)(cy / a.rows);
    dst[i] = src[c * a.sc + y * a.sy + x * a.sx];
}

// rgba [n][4] (4-byte aligned) -> dst [3][n]; table[colour * 256 + alpha]
__global__ __launch_bounds__(256) void image_composite_kernel(size_t n, const uint32_t* __restrict__ rgba, const uint8_t* __restrict__ table,
                                                              uint8_t* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t px = rgba[i], al = px >> 24;                              // little endian: r g b a
    dst[i] = table[((px & 0xFFu) << 8) | al];
    dst[n + i] = table[(((px >> 8) & 0xFFu) << 8) | al];
    dst[2 * n + i] = table[(((px >> 16) & 0xFFu) << 8) | al];
}

// ---- decode ---------------------------------------------------------------------------------------------------------------------------
constexpr int DQ = 4;                     // pixels per thread

__device__ __forceinline__ float unit(uint8_t b) { return __fdiv_rn((float)b, 255.f); }       // torch: uint8_tensor / 255.0 in float32

__device__ __forceinline__ void load4(const uint8_t* __restrict__ p, size_t at, int n, uint8_t v[DQ])
{
    if (n == DQ && ((reinterpret_cast<uintptr_t>(p) + at) & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + at);
        v[0] = (uint8_t)w; v[1] = (uint8_t)(w >> 8); v[2] = (uint8_t)(w >> 16); v[3] = (uint8_t)(w >> 24);
    } else {
#pragma unroll
        for (int j = 0; j < DQ; ++j) v[j] = j < n ? p[at + j] : (uint8_t)0;
    }
}

__device__ __forceinline__ void store4(float* __restrict__ p, size_t at, int n, const float v[DQ])
{
    if (n == DQ && ((reinterpret_cast<uintptr_t>(p + at)) & 15) == 0) {
        *reinterpret_cast<float4*>(p + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < DQ; ++j) if (j < n) p[at + j] = v[j];
    }
}

__global__ __launch_bounds__(256) void view_decode_kernel(MrgsViewDecode a, size_t HW, size_t HWg)
{
    const size_t at = ((size_t)blockIdx.x * 256 + threadIdx.x) * DQ;
    uint8_t b[3][DQ];
    float f[DQ];
    if (at < HW) {
        const int n = (int)(HW - at < (size_t)DQ ? HW - at : (size_t)DQ);
        if (a.gt) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                load4(a.rgb + c * HW, at, n, b[c]);
#pragma unroll
                for (int j = 0; j < DQ; ++j) f[j] = unit(b[c][j]);
                store4(a.gt + c * HW, at, n, f);
            }
        }
        if (a.alpha_out) {
            load4(a.alpha, at, n, b[0]);
#pragma unroll
            for (int j = 0; j < DQ; ++j) f[j] = unit(b[0][j]);
            store4(a.alpha_out, at, n, f);
        }
        if (a.mask_out) {                                                     // (img[..., -1] > 128).astype(float32), [H W, 1]
            load4(a.mask, at, n, b[0]);
#pragma unroll
            for (int j = 0; j < DQ; ++j) f[j] = b[0][j] > 128 ? 1.f : 0.f;
            store4(a.mask_out, at, n, f);
        }
        if (a.score_out) {                                                    // ref_score > 128 as a bool byte, [1, H, W]
            load4(a.score, at, n, b[0]);
            if (n == DQ && ((reinterpret_cast<uintptr_t>(a.score_out) + at) & 3) == 0)
                *reinterpret_cast<uint32_t*>(a.score_out + at) = (b[0][0] > 128 ? 1u : 0u) | (b[0][1] > 128 ? 0x100u : 0u) |
                                                                 (b[0][2] > 128 ? 0x10000u : 0u) | (b[0][3] > 128 ? 0x1000000u : 0u);
            else
                for (int j = 0; j < n; ++j) a.score_out[at + j] = b[0][j] > 128 ? 1 : 0;
        }
        if (a.normal_out) {                                                   // [H W, 3] pixel-interleaved in and out: 12 bytes -> 12 floats
            const uint8_t* __restrict__ s = a.normal + 3 * at;
            float* __restrict__ o = a.normal_out + 3 * at;
            if (n == DQ && (reinterpret_cast<uintptr_t>(s) & 3) == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t w = reinterpret_cast<const uint32_t*>(s)[q];
                    reinterpret_cast<float4*>(o)[q] = make_float4(a.normal_table[w & 0xFFu], a.normal_table[(w >> 8) & 0xFFu],
                                                                  a.normal_table[(w >> 16) & 0xFFu], a.normal_table[w >> 24]);
                }
            } else {
                for (int j = 0; j < 3 * n; ++j) o[j] = a.normal_table[s[j]];
            }
        }
    }
    if (a.grey && at < HWg) {
        // (0.299 r + 0.587 g) + 0.114 b on r, g, b = u8 / 255: utils/camera_utils.py:37, four roundings after the divisions
        const int n = (int)(HWg - at < (size_t)DQ ? HWg - at : (size_t)DQ);
#pragma unroll
        for (int c = 0; c < 3; ++c) load4(a.grey_rgb + c * HWg, at, n, b[c]);
#pragma unroll
        for (int j = 0; j < DQ; ++j)
            f[j] = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, unit(b[0][j])), __fmul_rn(0.587f, unit(b[1][j]))), __fmul_rn(0.114f, unit(b[2][j])));
        store4(a.grey, at, n, f);
    }
}

bool bad_size(int64_t v) { return v <= 0 || v > (1 << 24); }

}   // namespace

extern "C" size_t mrgs_image_resize_ws_bytes(int32_t channels, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w)
{
    if (channels <= 0 || bad_size(in_h) || bad_size(in_w) || bad_size(out_h) || bad_size(out_w)) return 0;
    return (in_w != out_w && in_h != out_h) ? (size_t)channels * in_h * out_w : 0;      // the 8-bit intermediate of two passes
}

extern "C" int mrgs_image_resize_u8(const MrgsResizeConfig* cfg, const uint8_t* src, const int32_t* bounds_x, const int32_t* kk_x,
                                    const int32_t* bounds_y, const int32_t* kk_y, void* ws, size_t ws_bytes, uint8_t* dst, void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsResizeConfig) || cfg->flags != 0) return MRGS_E_BAD_ARG;
    const int C = cfg->channels, ih = cfg->in_h, iw = cfg->in_w, oh = cfg->out_h, ow = cfg->out_w;
    if (C < 1 || C > 4 || bad_size(ih) || bad_size(iw) || bad_size(oh) || bad_size(ow) || !src || !dst) return MRGS_E_BAD_ARG;
    if (cfg->stride_c < 0 || cfg->stride_y <= 0 || cfg->stride_x <= 0) return MRGS_E_BAD_ARG;
    const bool px = iw != ow, py = ih != oh;
    if (px && (!bounds_x || !kk_x || cfg->ksize_x < 1)) return MRGS_E_BAD_ARG;
    if (py && (!bounds_y || !kk_y || cfg->ksize_y < 1)) return MRGS_E_BAD_ARG;
    const size_t tmp_bytes = mrgs_image_resize_ws_bytes(C, ih, iw, oh, ow);
    if (tmp_bytes && !ws) return MRGS_E_BAD_ARG;
    if (ws_bytes < tmp_bytes) return MRGS_E_WORKSPACE;
    const size_t most = (size_t)C * (size_t)(ih > oh ? ih : oh) * (size_t)(iw > ow ? iw : ow);
    if ((most + 255) / 256 > 0x7fffffffu) return MRGS_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    auto blocks = [](size_t n) { return (unsigned)((n + 255) / 256); };
    ResizeArgs a;
    a.C = C; a.sc = cfg->stride_c; a.sy = cfg->stride_y; a.sx = cfg->stride_x;
    if (!px && !py) {
        a.rows = ih; a.in_len = iw; a.out_len = iw; a.ksize = 0;
        image_gather_kernel<<<blocks((size_t)C * ih * iw), 256, 0, st>>>(a, src, dst);
        return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
    }
    const uint8_t* from = src;
    if (px) {                                                               // horizontal first, over every source row
        uint8_t* to = py ? (uint8_t*)ws : dst;
        a.rows = ih; a.in_len = iw; a.out_len = ow; a.ksize = cfg->ksize_x;
        image_resize_h_kernel<<<blocks((size_t)C * ih * ow), 256, 0, st>>>(a, from, bounds_x, kk_x, to);
        from = to; a.sc = (int64_t)ih * ow; a.sy = ow; a.sx = 1;
    }
    if (py) {
        a.rows = ow; a.in_len = ih; a.out_len = oh; a.ksize = cfg->ksize_y;
        image_resize_v_kernel<<<blocks((size_t)C * oh * ow), 256, 0, st>>>(a, from, bounds_y, kk_y, dst);
    }
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}

extern "C" int mrgs_image_composite_u8(int64_t n_pixels, const uint8_t* rgba, const uint8_t* table, uint8_t* dst, void* stream)
{
    if (n_pixels < 0 || n_pixels >= ((int64_t)1 << 36)) return MRGS_E_BAD_ARG;
    if (n_pixels == 0) return MRGS_OK;
    if (!rgba || !table || !dst || (reinterpret_cast<uintptr_t>(rgba) & 3)) return MRGS_E_BAD_ARG;
    image_composite_kernel<<<(unsigned)((n_pixels + 255) / 256), 256, 0, (hipStream_t)stream>>>((size_t)n_pixels, (const uint32_t*)rgba, table, dst);
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}

extern "C" int mrgs_view_decode(const MrgsViewDecode* v, void* stream)
{
    if (!v || v->struct_size != sizeof(MrgsViewDecode) || v->flags != 0 || bad_size(v->H) || bad_size(v->W)) return MRGS_E_BAD_ARG;
    if (!v->gt && !v->alpha_out && !v->grey && !v->normal_out && !v->mask_out && !v->score_out) return MRGS_E_BAD_ARG;
    if ((v->gt && !v->rgb) || (v->alpha_out && !v->alpha) || (v->mask_out && !v->mask) || (v->score_out && !v->score)) return MRGS_E_BAD_ARG;
    if (v->normal_out && (!v->normal || !v->normal_table)) return MRGS_E_BAD_ARG;
    if (v->grey && (!v->grey_rgb || bad_size(v->Hg) || bad_size(v->Wg))) return MRGS_E_BAD_ARG;
    for (const float* p : {(const float*)v->gt, (const float*)v->alpha_out, (const float*)v->grey, (const float*)v->normal_out,
                           (const float*)v->mask_out, v->normal_table})
        if (reinterpret_cast<uintptr_t>(p) & 3) return MRGS_E_BAD_ARG;
    const size_t HW = (size_t)v->H * v->W, HWg = v->grey ? (size_t)v->Hg * v->Wg : 0;
    const bool image_side = v->gt || v->alpha_out || v->normal_out || v->mask_out || v->score_out;
    const size_t most = image_side ? (HW > HWg ? HW : HWg) : HWg;
    const size_t quads = (most + DQ - 1) / DQ;
    if ((quads + 255) / 256 > 0x7fffffffu) return MRGS_E_UNSUPPORTED;
    view_decode_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, (hipStream_t)stream>>>(*v, image_side ? HW : 0, HWg);
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}
