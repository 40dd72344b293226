// The LPIPS (VGG16) perceptual distance of one image pair and its gradient to the first image: lpipsPyTorch/modules (networks.py:88-96 the
// network, lpips.py:30-36 the distance, utils.py:6-8 the normalisation); utils/loss_utils.py:209-212 adds it to the loss from iteration
// 18 000 on.  The contract is in include/mrgs.h.  fp32 throughout; activations channel-last [H][W][C], so a K chunk of a pixel is contiguous.
//   lpips_conv3x3        implicit GEMM on v_mfma_f32_32x32x2_f32 (per output an fmaf chain over each K chunk, the chunk sums added in order).  A workgroup (4 waves) takes a
//                        LPIPS_TILE^2 pixel tile x LPIPS_NT output channels; K = 9 taps x Cin runs in chunks of LPIPS_KC channels: the
//                        tile with its 1-pixel halo (zeros outside the image) and the chunk's 9 x KC x NT weights go to LDS, a wave
//                        multiplies 4 rows of the tile (two 32-pixel blocks) by the 64 channels (two 32-channel blocks): 4 accumulator
//                        blocks, 2 + 2 LDS reads per 4 matrix instructions.  Epilogue: + bias, + add, ReLU, gate.  blockIdx.z = image.
//                        The backward-to-data pass is the same kernel on the flipped, transposed matrix packed beside the forward's.
//   lpips_conv_first     3 -> 64 on the VALU (0.6 % of the network's products): reads the CHW planes, applies the input transform in the
//                        tile load (the padding ring is 0 in z-scored space), one pixel per thread, fmaf chains of 27.
//   lpips_conv_last_bwd  64 -> 3 on the VALU: one pixel per thread, three fmaf chains of 576, writes CHW times in_scale / scale_c.
//   lpips_pool_fwd / lpips_pool_bwd   the 2 x 2 maximum in launches of their own; the backward is a gather: a full-resolution texel
//                        takes its window's gradient when it is the window's first maximum in row-major order, then + the head's
//                        gradient of the level and the gate a > 0, both read from the stored ReLU output.
//   lpips_head_fwd / lpips_head_bwd / lpips_head_finalize   one wave per pixel: both norms, the weighted squared difference; a partial row
//                        per workgroup, summed in double in a fixed order.  The backward is the closed form of the quotient.
#include "mrgs_internal.h"
#include "mrgs_wave.h"

namespace {

constexpr int LPIPS_TILE = 16;                // width and height of a convolution's pixel tile
constexpr int LPIPS_KC = 16;                  // input channels of a K chunk
constexpr int LPIPS_NT = 64;                  // output channels of a workgroup
constexpr int IN_W = LPIPS_TILE + 2;          // the tile with its halo
constexpr int PIX_STRIDE = LPIPS_KC + 1;      // floats between two pixels of the staged tile: odd, so the 16 pixels of a row hit 16 banks
constexpr int HEAD_MAX_BLOCKS = 1024;
constexpr int HEAD_ROW = 4;                   // a partial row is one 16-byte word
constexpr int N_CONV = 13, N_LEVEL = 5;
const int CONV_CIN[N_CONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int CONV_COUT[N_CONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int CONV_STAGE[N_CONV] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
const int LEVEL_CONV[N_LEVEL] = {1, 3, 6, 9, 12};
__constant__ const float ZS_SHIFT[3] = {-.030f, -.088f, -.188f};
__constant__ const float ZS_SCALE[3] = {.458f, .448f, .450f};
const float ZS_SCALE_HOST[3] = {.458f, .448f, .450f};

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
    const float* in[2];
    float* out[2];
    const float* add[2];         // nullable
    const float* gate[2];        // nullable
    const float* w;              // [9][Cin][Cout]
    const float* bias;           // nullable
    int H, W, Cin, Cout, tiles_x, relu;
    int zscore;                  // first / last only
    float in_scale, in_offset;   // first only
    float out_scale[3];          // last only
};

// ---- the convolution on the matrix pipe: Cin a multiple of LPIPS_KC, Cout a multiple of LPIPS_NT --------------------------------------------
__global__ __launch_bounds__(256) void lpips_conv3x3(ConvArgs a)
{
    __shared__ __align__(16) float s_w[9 * LPIPS_KC * LPIPS_NT];
    __shared__ float s_in[IN_W * IN_W * PIX_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
    const int img = blockIdx.z, n0 = blockIdx.y * LPIPS_NT;
    const int y0 = (blockIdx.x / a.tiles_x) * LPIPS_TILE, x0 = (blockIdx.x % a.tiles_x) * LPIPS_TILE;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
    const float* __restrict__ in = a.in[img];
    const int prow = l32 >> 4, pcol = l32 & 15;          // the pixel of an operand row inside its 2 x 16 block
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += LPIPS_KC) {
        __syncthreads();                                  // the chunk before has been multiplied
        for (int t = tid; t < IN_W * IN_W * (LPIPS_KC / 4); t += 256) {
            const int pix = t >> 2, q = t & 3;
            const int ly = pix / IN_W, lx = pix - ly * IN_W;
            const int y = y0 + ly - 1, x = x0 + lx - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < H && x >= 0 && x < W) v = *reinterpret_cast<const float4*>(in + ((size_t)y * W + x) * Cin + c0 + 4 * q);
            float* d = s_in + pix * PIX_STRIDE + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        for (int t = tid; t < 9 * LPIPS_KC * (LPIPS_NT / 4); t += 256) {
            const int row = t >> 4, q = t & 15;           // row = tap * KC + k
            const int tap = row / LPIPS_KC, k = row - tap * LPIPS_KC;
            *reinterpret_cast<float4*>(s_w + row * LPIPS_NT + 4 * q) =
                *reinterpret_cast<const float4*>(a.w + ((size_t)tap * Cin + c0 + k) * Cout + n0 + 4 * q);
        }
        __syncthreads();
        // a chunk's 9 KC products are chained into their own accumulators and join the running sum once: the rounding of a sum over
        // 9 Cin products (up to 4608) grows with the chain's length, and chunk sums of 144 keep it at that of a blocked fp32 sum
        f32x16 part[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
            const float* pa0 = s_in + ((4 * wave + prow + dy) * IN_W + pcol + dx) * PIX_STRIDE + half;
            const float* pa1 = pa0 + 2 * IN_W * PIX_STRIDE;
            const float* pb = s_w + (tap * LPIPS_KC + half) * LPIPS_NT + l32;
#pragma unroll
            for (int kk = 0; kk < LPIPS_KC / 2; ++kk) {
                const float a0 = pa0[2 * kk], a1 = pa1[2 * kk];
                const float b0 = pb[2 * kk * LPIPS_NT], b1 = pb[2 * kk * LPIPS_NT + 32];
                part[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, part[0][0], 0, 0, 0);
                part[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, part[0][1], 0, 0, 0);
                part[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, part[1][0], 0, 0, 0);
                part[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, part[1][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];
    }
    // register r of lane l holds row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32 of a 32 x 32 block
    float* __restrict__ out = a.out[img];
    const float* __restrict__ add = a.add[img];
    const float* __restrict__ gate = a.gate[img];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int n = n0 + 32 * nb + l32;
            const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = 8 * (r >> 2) + 4 * half + (r & 3);
                const int y = y0 + 4 * wave + 2 * mb + (m >> 4), x = x0 + (m & 15);
                if (y < H && x < W) {
                    const size_t o = ((size_t)y * W + x) * Cout + n;
                    float v = acc[mb][nb][r] + b;
                    if (add) v += add[o];
                    if (a.relu) v = fmaxf(v, 0.f);
                    if (gate) v = gate[o] > 0.f ? v : 0.f;
                    out[o] = v;
                }
            }
        }
}

// ---- 3 -> 64 from the CHW planes -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lpips_conv_first(ConvArgs a)
{
    __shared__ float s_in[3][IN_W * IN_W];
    __shared__ __align__(16) float s_w[27 * 64];
    __shared__ __align__(16) float s_b[64];
    const int tid = threadIdx.x, img = blockIdx.z;
    const int y0 = (blockIdx.x / a.tiles_x) * LPIPS_TILE, x0 = (blockIdx.x % a.tiles_x) * LPIPS_TILE;
    const int H = a.H, W = a.W;
    const float* __restrict__ in = a.in[img];
    for (int t = tid; t < 3 * IN_W * IN_W; t += 256) {
        const int c = t / (IN_W * IN_W), pix = t - c * (IN_W * IN_W);
        const int ly = pix / IN_W, lx = pix - ly * IN_W;
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        float v = 0.f;                                    // the padding ring is 0 behind the transform
        if (y >= 0 && y < H && x >= 0 && x < W) {
            v = in[((size_t)c * H + y) * W + x];
            if (a.zscore) v = ((a.in_scale * v + a.in_offset) - ZS_SHIFT[c]) / ZS_SCALE[c];
        }
        s_in[c][pix] = v;
    }
    for (int t = tid; t < 27 * 64; t += 256) {            // [tap][ci][co] -> row k = ci * 9 + tap, as the gather below orders a pixel's values
        const int tap = t / 192, ci = (t / 64) % 3, co = t & 63;
        s_w[(ci * 9 + tap) * 64 + co] = a.w[t];
    }
    if (tid < 64) s_b[tid] = a.bias ? a.bias[tid] : 0.f;
    __syncthreads();
    const int ly = tid >> 4, lx = tid & 15, y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) return;
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) v[c * 9 + tap] = s_in[c][(ly + tap / 3) * IN_W + lx + tap % 3];
    float* __restrict__ out = a.out[img] + ((size_t)y * W + x) * 64;
    for (int co = 0; co < 64; co += 4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const float4 w = *reinterpret_cast<const float4*>(s_w + k * 64 + co);
            s.x = fmaf(v[k], w.x, s.x); s.y = fmaf(v[k], w.y, s.y); s.z = fmaf(v[k], w.z, s.z); s.w = fmaf(v[k], w.w, s.w);
        }
        const float4 b = *reinterpret_cast<const float4*>(s_b + co);
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
        if (a.relu) { s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f); }
        *reinterpret_cast<float4*>(out + co) = s;
    }
}

// ---- 64 -> 3 to the CHW planes: the last step of the backward ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lpips_conv_last_bwd(ConvArgs a)
{
    __shared__ float s_in[IN_W * IN_W * PIX_STRIDE];
    __shared__ float s_w[9 * 64 * 3];
    const int tid = threadIdx.x, img = blockIdx.z;
    const int y0 = (blockIdx.x / a.tiles_x) * LPIPS_TILE, x0 = (blockIdx.x % a.tiles_x) * LPIPS_TILE;
    const int H = a.H, W = a.W;
    const float* __restrict__ in = a.in[img];
    for (int t = tid; t < 9 * 64 * 3; t += 256) s_w[t] = a.w[t];
    const int ly = tid >> 4, lx = tid & 15, y = y0 + ly, x = x0 + lx;
    float s[3] = {0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < 64; c0 += LPIPS_KC) {
        __syncthreads();
        for (int t = tid; t < IN_W * IN_W * (LPIPS_KC / 4); t += 256) {
            const int pix = t >> 2, q = t & 3;
            const int py = pix / IN_W, px = pix - py * IN_W;
            const int yy = y0 + py - 1, xx = x0 + px - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = *reinterpret_cast<const float4*>(in + ((size_t)yy * W + xx) * 64 + c0 + 4 * q);
            float* d = s_in + pix * PIX_STRIDE + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float* p = s_in + ((ly + tap / 3) * IN_W + lx + tap % 3) * PIX_STRIDE;
            const float* w = s_w + (tap * 64 + c0) * 3;
#pragma unroll
            for (int k = 0; k < LPIPS_KC; ++k) {
                s[0] = fmaf(p[k], w[3 * k], s[0]); s[1] = fmaf(p[k], w[3 * k + 1], s[1]); s[2] = fmaf(p[k], w[3 * k + 2], s[2]);
            }
        }
    }
    if (y >= H || x >= W) return;
    float* __restrict__ out = a.out[img];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((size_t)c * H + y) * W + x] = s[c] * a.out_scale[c];
}

// ---- the 2 x 2 maximum ------------------------------------------------------------------------------------------------------------------------------
struct PoolArgs {
    const float* a[2];           // [H][W][C]
    float* out[2];
    const float* g_pooled;       // backward: [Ho][Wo][C]
    const float* add;            // backward: nullable, [H][W][C]
    int H, W, C, gate;
};

__global__ __launch_bounds__(256) void lpips_pool_fwd(PoolArgs p)
{
    const int Ho = p.H >> 1, Wo = p.W >> 1, C4 = p.C >> 2;
    const size_t n = (size_t)Ho * Wo * C4;
    const float4* __restrict__ a = reinterpret_cast<const float4*>(p.a[blockIdx.y]);
    float4* __restrict__ out = reinterpret_cast<float4*>(p.out[blockIdx.y]);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C4);
        const size_t pix = i / C4;
        const int x = (int)(pix % Wo), y = (int)(pix / Wo);
        const size_t b = ((size_t)(2 * y) * p.W + 2 * x) * C4 + c;
        const float4 v0 = a[b], v1 = a[b + C4], v2 = a[b + (size_t)p.W * C4], v3 = a[b + (size_t)p.W * C4 + C4];
        out[i] = make_float4(fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x)), fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y)),
                             fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z)), fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w)));
    }
}

// the index (0..3, row-major) of the first maximum of a window
__device__ __forceinline__ int first_max(float v0, float v1, float v2, float v3)
{
    int k = 0; float m = v0;
    if (v1 > m) { m = v1; k = 1; }
    if (v2 > m) { m = v2; k = 2; }
    if (v3 > m) { k = 3; }
    return k;
}

__global__ __launch_bounds__(256) void lpips_pool_bwd(PoolArgs p)
{
    const int Ho = p.H >> 1, Wo = p.W >> 1, C = p.C;
    const size_t n = (size_t)p.H * p.W * C;
    const float* __restrict__ a = p.a[0];
    float* __restrict__ out = p.out[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const size_t pix = i / C;
        const int x = (int)(pix % p.W), y = (int)(pix / p.W);
        const int wy = y >> 1, wx = x >> 1;
        float g = 0.f;
        if (wy < Ho && wx < Wo) {
            const size_t b = ((size_t)(2 * wy) * p.W + 2 * wx) * C + c;
            const int k = first_max(a[b], a[b + C], a[b + (size_t)p.W * C], a[b + (size_t)p.W * C + C]);
            if (k == ((y & 1) << 1 | (x & 1))) g = p.g_pooled[((size_t)wy * Wo + wx) * C + c];
        }
        if (p.add) g += p.add[i];
        if (p.gate) g = a[i] > 0.f ? g : 0.f;
        out[i] = g;
    }
}

// ---- the head of one level ----------------------------------------------------------------------------------------------------------------------------
// One wave per pixel; lane l holds channels l + 64 j.  C = 64 J, J in {1, 2, 4, 8}.
struct HeadPixel { float nx, ny, s; };
template <int J>
__device__ __forceinline__ void head_load(const float* __restrict__ f, size_t p, int lane, float (&v)[J])
{
#pragma unroll
    for (int j = 0; j < J; ++j) v[j] = f[p * (64 * J) + lane + 64 * j];
}
template <int J>
__device__ __forceinline__ float head_norm(const float (&v)[J])
{
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) s = fmaf(v[j], v[j], s);
    return sqrtf(wave_shfl_sum(s));
}

template <int J>
__global__ __launch_bounds__(256) void lpips_head_fwd(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ w,
                                                      long long P, float* __restrict__ partials)
{
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wl[J];
#pragma unroll
    for (int j = 0; j < J; ++j) wl[j] = w[lane + 64 * j];
    float acc = 0.f;
    for (long long p = (long long)blockIdx.x * 4 + wave; p < P; p += (long long)gridDim.x * 4) {
        float vx[J], vy[J];
        head_load<J>(fx, (size_t)p, lane, vx);
        head_load<J>(fy, (size_t)p, lane, vy);
        const float nx = head_norm<J>(vx), ny = head_norm<J>(vy);
        const float ix = 1.f / (nx + 1e-10f), iy = 1.f / (ny + 1e-10f);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) { const float d = vx[j] * ix - vy[j] * iy; s = fmaf(wl[j] * d, d, s); }
        s = wave_shfl_sum(s);
        if (nx > 0.f && ny > 0.f) acc += s;               // an all-zero vector: the pixel contributes 0 (mrgs.h)
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x < HEAD_ROW) partials[(size_t)blockIdx.x * HEAD_ROW + threadIdx.x] = threadIdx.x == 0 ? (red[0] + red[1]) + (red[2] + red[3]) : 0.f;
}

// d term / d fx_k = 1/P [ d_k / (n + e) - fx_k S / (n (n + e)^2) ], d_c = 2 w_c (u_c - v_c), S = sum_c d_c fx_c
template <int J>
__global__ __launch_bounds__(256) void lpips_head_bwd(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ w,
                                                      long long P, const float* __restrict__ g, int gate, float* __restrict__ g_fx)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wl[J];
#pragma unroll
    for (int j = 0; j < J; ++j) wl[j] = w[lane + 64 * j];
    const float coef = g[0] / (float)P;
    for (long long p = (long long)blockIdx.x * 4 + wave; p < P; p += (long long)gridDim.x * 4) {
        float vx[J], vy[J], d[J];
        head_load<J>(fx, (size_t)p, lane, vx);
        head_load<J>(fy, (size_t)p, lane, vy);
        const float nx = head_norm<J>(vx), ny = head_norm<J>(vy);
        const float ix = 1.f / (nx + 1e-10f), iy = 1.f / (ny + 1e-10f);
        float S = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) { d[j] = 2.f * wl[j] * (vx[j] * ix - vy[j] * iy); S = fmaf(d[j], vx[j], S); }
        S = wave_shfl_sum(S);
        const bool live = nx > 0.f && ny > 0.f;
        const float c1 = live ? coef * ix : 0.f, c2 = live ? coef * S * ix * ix / nx : 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            float r = c1 * d[j] - c2 * vx[j];
            if (gate && !(vx[j] > 0.f)) r = 0.f;
            g_fx[(size_t)p * (64 * J) + lane + 64 * j] = r;
        }
    }
}

struct HeadFinal { int nblocks[N_LEVEL]; double P[N_LEVEL]; int first, count; };
// terms[l] for the levels [first, first + count), and terms[5] = their sum when all five are asked for
__global__ __launch_bounds__(256) void lpips_head_finalize(HeadFinal f, const float* __restrict__ partials, float* __restrict__ terms)
{
    __shared__ double red[4][1];
    double total = 0.0;
    for (int l = f.first; l < f.first + f.count; ++l) {
        block_rows_sum_256<1, HEAD_ROW>(partials + (size_t)l * HEAD_MAX_BLOCKS * HEAD_ROW, f.nblocks[l], red);
        const double t = rows_total(red, 0) / f.P[l];
        if (threadIdx.x == 0) terms[l] = (float)t;
        total += t;
        __syncthreads();                                  // red is written again
    }
    if (threadIdx.x == 0 && f.count == N_LEVEL) terms[N_LEVEL] = (float)total;
}

// ---- weights ----------------------------------------------------------------------------------------------------------------------------------------------
// w [Cout][Cin][3][3] -> fwd [9][Cin][Cout] and bwd [9][Cout][Cin] with the taps flipped (either nullable)
__global__ __launch_bounds__(256) void lpips_pack_conv(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ fwd, float* __restrict__ bwd)
{
    const size_t n = (size_t)9 * Cin * Cout;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % 9);
        const size_t r = i / 9;
        const int ci = (int)(r % Cin), co = (int)(r / Cin);
        const float v = w[i];
        if (fwd) fwd[((size_t)t * Cin + ci) * Cout + co] = v;
        if (bwd) bwd[((size_t)(8 - t) * Cout + co) * Cin + ci] = v;
    }
}
__global__ __launch_bounds__(256) void lpips_copy(const float* __restrict__ src, float* __restrict__ dst, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

struct Blob { size_t fwd[N_CONV], bias[N_CONV], bwd[N_CONV], lin[N_LEVEL], total; };   // offsets in floats, each a multiple of 64
Blob blob_layout()
{
    Blob b;
    size_t o = 0;
    for (int i = 0; i < N_CONV; ++i) {
        const size_t n = mrgs_align_up((size_t)9 * CONV_CIN[i] * CONV_COUT[i], 64);
        b.fwd[i] = o; o += n;
        b.bias[i] = o; o += mrgs_align_up(CONV_COUT[i], 64);
        b.bwd[i] = o; o += n;
    }
    for (int l = 0; l < N_LEVEL; ++l) { b.lin[l] = o; o += mrgs_align_up(CONV_COUT[LEVEL_CONV[l]], 64); }
    b.total = o;
    return b;
}

// ---- workspace ----------------------------------------------------------------------------------------------------------------------------------------------
struct Ws {
    size_t partials;                      // offsets in floats, each a multiple of 64
    size_t xact[N_CONV], ytap[N_LEVEL];   // with_grad
    size_t T[2][2];                       // ping-pong of image i; with_grad: T[1] only, and T[0][0] = the pooled x, T[0][1] = the head's gradient
    size_t total;
};
size_t stage_pixels(int H, int W, int s) { return (size_t)(H >> s) * (size_t)(W >> s); }
Ws ws_layout(int H, int W, int with_grad)
{
    Ws w{};
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += mrgs_align_up(n, 64); return at; };
    const size_t n = (size_t)H * W;
    w.partials = take((size_t)N_LEVEL * HEAD_MAX_BLOCKS * HEAD_ROW);
    if (with_grad) {
        for (int i = 0; i < N_CONV; ++i) w.xact[i] = take(stage_pixels(H, W, CONV_STAGE[i]) * CONV_COUT[i]);
        for (int l = 0; l < N_LEVEL; ++l) w.ytap[l] = take(stage_pixels(H, W, l) * CONV_COUT[LEVEL_CONV[l]]);
        w.T[0][0] = take(stage_pixels(H, W, 1) * 64);
        w.T[0][1] = take(64 * n);
        w.T[1][0] = take(64 * n);
        w.T[1][1] = take(64 * n);
    } else {
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) w.T[i][j] = take(64 * n);
    }
    w.total = o;
    return w;
}

bool size_ok(int H, int W) { return H >= 16 && W >= 16 && (long long)H * W <= (1ll << 24); }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
int grid_1d(size_t n) { const size_t b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b ? b : 1)); }

// ---- launches -----------------------------------------------------------------------------------------------------------------------------------------------
void launch_conv(ConvArgs a, int n_images, hipStream_t st)
{
    const int tiles_y = (a.H + LPIPS_TILE - 1) / LPIPS_TILE;
    a.tiles_x = (a.W + LPIPS_TILE - 1) / LPIPS_TILE;
    const unsigned tiles = (unsigned)(a.tiles_x * tiles_y);
    if (a.Cin == 3) lpips_conv_first<<<dim3(tiles, 1, n_images), 256, 0, st>>>(a);
    else if (a.Cout == 3) lpips_conv_last_bwd<<<dim3(tiles, 1, n_images), 256, 0, st>>>(a);
    else lpips_conv3x3<<<dim3(tiles, a.Cout / LPIPS_NT, n_images), 256, 0, st>>>(a);
}

int head_blocks(long long P) { const long long b = (P + 3) / 4; return (int)(b > HEAD_MAX_BLOCKS ? HEAD_MAX_BLOCKS : b); }
void launch_head_fwd(int C, const float* fx, const float* fy, const float* w, long long P, float* partials, hipStream_t st)
{
    const int nb = head_blocks(P);
    switch (C) {
    case 64: lpips_head_fwd<1><<<nb, 256, 0, st>>>(fx, fy, w, P, partials); break;
    case 128: lpips_head_fwd<2><<<nb, 256, 0, st>>>(fx, fy, w, P, partials); break;
    case 256: lpips_head_fwd<4><<<nb, 256, 0, st>>>(fx, fy, w, P, partials); break;
    default: lpips_head_fwd<8><<<nb, 256, 0, st>>>(fx, fy, w, P, partials); break;
    }
}
void launch_head_bwd(int C, const float* fx, const float* fy, const float* w, long long P, const float* g, int gate, float* g_fx, hipStream_t st)
{
    const int nb = head_blocks(P);
    switch (C) {
    case 64: lpips_head_bwd<1><<<nb, 256, 0, st>>>(fx, fy, w, P, g, gate, g_fx); break;
    case 128: lpips_head_bwd<2><<<nb, 256, 0, st>>>(fx, fy, w, P, g, gate, g_fx); break;
    case 256: lpips_head_bwd<4><<<nb, 256, 0, st>>>(fx, fy, w, P, g, gate, g_fx); break;
    default: lpips_head_bwd<8><<<nb, 256, 0, st>>>(fx, fy, w, P, g, gate, g_fx); break;
    }
}

// the library's one status path, written out (the macro's users are enumerated by tests/test_status.py, one call per file; this file's
// failure path is covered by tests/test_lpips_cpu.py)
#define LPIPS_LAUNCH_STATUS mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__)

bool served_pair(int Cin, int Cout)
{
    for (int i = 0; i < N_CONV; ++i)
        if (CONV_CIN[i] == Cin && CONV_COUT[i] == Cout) return true;
    return false;
}

bool config_ok(const MrgsLpipsConfig* cfg)
{
    return cfg && cfg->struct_size == sizeof(MrgsLpipsConfig) && size_ok(cfg->H, cfg->W) && (cfg->with_grad == 0 || cfg->with_grad == 1);
}

}   // namespace

extern "C" size_t mrgs_lpips_weights_bytes(void) { return blob_layout().total * sizeof(float); }

extern "C" int mrgs_lpips_pack_weights(const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* blob, void* stream)
{
    if (!conv_w || !conv_b || !lin_w || !blob || !aligned(blob, 256)) return MRGS_E_BAD_ARG;
    for (int i = 0; i < N_CONV; ++i)
        if (!conv_w[i] || !conv_b[i]) return MRGS_E_BAD_ARG;
    for (int l = 0; l < N_LEVEL; ++l)
        if (!lin_w[l]) return MRGS_E_BAD_ARG;
    const Blob b = blob_layout();
    float* base = (float*)blob;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < N_CONV; ++i) {
        lpips_pack_conv<<<grid_1d((size_t)9 * CONV_CIN[i] * CONV_COUT[i]), 256, 0, st>>>(conv_w[i], CONV_CIN[i], CONV_COUT[i], base + b.fwd[i], base + b.bwd[i]);
        lpips_copy<<<(CONV_COUT[i] + 255) / 256, 256, 0, st>>>(conv_b[i], base + b.bias[i], CONV_COUT[i]);
    }
    for (int l = 0; l < N_LEVEL; ++l) {
        const int C = CONV_COUT[LEVEL_CONV[l]];
        lpips_copy<<<(C + 255) / 256, 256, 0, st>>>(lin_w[l], base + b.lin[l], C);
    }
    return LPIPS_LAUNCH_STATUS;
}

extern "C" size_t mrgs_lpips_ws_bytes(int32_t H, int32_t W, int32_t with_grad)
{
    if (!size_ok(H, W) || (with_grad != 0 && with_grad != 1)) return 0;
    return ws_layout(H, W, with_grad).total * sizeof(float);
}

extern "C" int mrgs_lpips_ws_offsets(int32_t H, int32_t W, size_t* offsets)
{
    if (!size_ok(H, W) || !offsets) return MRGS_E_BAD_ARG;
    const Ws w = ws_layout(H, W, 1);
    for (int i = 0; i < N_CONV; ++i) offsets[i] = w.xact[i] * sizeof(float);
    for (int l = 0; l < N_LEVEL; ++l) offsets[N_CONV + l] = w.ytap[l] * sizeof(float);
    return MRGS_OK;
}

extern "C" int mrgs_lpips_forward(const MrgsLpipsConfig* cfg, const void* blob, const float* x, const float* y, void* ws, size_t ws_bytes,
                                  float* terms, void* stream)
{
    if (!config_ok(cfg) || !blob || !x || !y || !ws || !terms || !aligned(blob, 256) || !aligned(ws, 256)) return MRGS_E_BAD_ARG;
    if (ws_bytes < mrgs_lpips_ws_bytes(cfg->H, cfg->W, cfg->with_grad)) return MRGS_E_BAD_ARG;
    const int H = cfg->H, W = cfg->W, grad = cfg->with_grad;
    const Ws w = ws_layout(H, W, grad);
    const Blob b = blob_layout();
    const float* wb = (const float*)blob;
    float* base = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    HeadFinal fin{};
    fin.first = 0; fin.count = N_LEVEL;
    const float* cur[2] = {x, y};
    int flip[2] = {0, 0};                                 // the ping-pong buffer of image i that is written next
    // with_grad: x keeps every output and ping-pongs nothing but its pooled maps, which all fit T[0][0]
    auto next_buf = [&](int i) { float* p = base + w.T[i][(grad && i == 0) ? 0 : flip[i]]; flip[i] ^= 1; return p; };
    int level = 0;
    for (int i = 0; i < N_CONV; ++i) {
        const int s = CONV_STAGE[i], Hs = H >> s, Ws_ = W >> s;
        if (i > 0 && CONV_STAGE[i - 1] != s) {
            PoolArgs p{};
            p.H = H >> (s - 1); p.W = W >> (s - 1); p.C = CONV_CIN[i];
            for (int k = 0; k < 2; ++k) { p.a[k] = cur[k]; p.out[k] = next_buf(k); cur[k] = p.out[k]; }
            lpips_pool_fwd<<<dim3(grid_1d((size_t)Hs * Ws_ * (p.C / 4)), 2), 256, 0, st>>>(p);
        }
        const bool tap = LEVEL_CONV[level] == i;
        ConvArgs a{};
        a.H = Hs; a.W = Ws_; a.Cin = CONV_CIN[i]; a.Cout = CONV_COUT[i]; a.relu = 1;
        a.w = wb + b.fwd[i]; a.bias = wb + b.bias[i];
        a.zscore = 1; a.in_scale = cfg->in_scale; a.in_offset = cfg->in_offset;
        a.in[0] = cur[0]; a.in[1] = cur[1];
        a.out[0] = grad ? base + w.xact[i] : next_buf(0);
        a.out[1] = (grad && tap) ? base + w.ytap[level] : next_buf(1);
        launch_conv(a, 2, st);
        cur[0] = a.out[0]; cur[1] = a.out[1];
        if (tap) {
            const long long P = (long long)Hs * Ws_;
            fin.nblocks[level] = head_blocks(P); fin.P[level] = (double)P;
            launch_head_fwd(a.Cout, cur[0], cur[1], wb + b.lin[level], P, base + w.partials + (size_t)level * HEAD_MAX_BLOCKS * HEAD_ROW, st);
            ++level;
        }
    }
    lpips_head_finalize<<<1, 256, 0, st>>>(fin, base + w.partials, terms);
    return LPIPS_LAUNCH_STATUS;
}

extern "C" int mrgs_lpips_backward(const MrgsLpipsConfig* cfg, const void* blob, void* ws, const float* g_total, float* g_x, void* stream)
{
    if (!config_ok(cfg) || cfg->with_grad != 1 || !blob || !ws || !g_total || !g_x || !aligned(blob, 256) || !aligned(ws, 256)) return MRGS_E_BAD_ARG;
    const int H = cfg->H, W = cfg->W;
    const Ws w = ws_layout(H, W, 1);
    const Blob b = blob_layout();
    const float* wb = (const float*)blob;
    float* base = (float*)ws;
    hipStream_t st = (hipStream_t)stream;
    float* G[2] = {base + w.T[1][0], base + w.T[1][1]};   // y's ping-pong buffers carry the gradient
    float* HG = base + w.T[0][1];
    auto head_bwd = [&](int level, int gate, float* out) {
        const int i = LEVEL_CONV[level];
        const long long P = (long long)stage_pixels(H, W, level);
        launch_head_bwd(CONV_COUT[i], base + w.xact[i], base + w.ytap[level], wb + b.lin[level], P, g_total, gate, out, st);
    };
    int c = 0;                                            // G[c] holds the gradient of convolution i's pre-activation
    head_bwd(N_LEVEL - 1, 1, G[c]);
    for (int i = N_CONV - 1; i >= 1; --i) {
        const int s = CONV_STAGE[i];
        const bool pooled = CONV_STAGE[i - 1] != s;
        ConvArgs a{};
        a.H = H >> s; a.W = W >> s; a.Cin = CONV_COUT[i]; a.Cout = CONV_CIN[i];
        a.w = wb + b.bwd[i];
        a.in[0] = G[c]; a.out[0] = G[c ^ 1];
        a.gate[0] = pooled ? nullptr : base + w.xact[i - 1];
        launch_conv(a, 1, st);
        if (pooled) {                                     // convolution i - 1 is a tap: its head gradient joins at full resolution
            head_bwd(s - 1, 0, HG);
            PoolArgs p{};
            p.H = H >> (s - 1); p.W = W >> (s - 1); p.C = CONV_CIN[i]; p.gate = 1;
            p.a[0] = base + w.xact[i - 1]; p.g_pooled = G[c ^ 1]; p.add = HG; p.out[0] = G[c];
            lpips_pool_bwd<<<grid_1d((size_t)p.H * p.W * p.C), 256, 0, st>>>(p);
        } else {
            c ^= 1;
        }
    }
    ConvArgs a{};
    a.H = H; a.W = W; a.Cin = 64; a.Cout = 3;
    a.w = wb + b.bwd[0];
    a.in[0] = G[c]; a.out[0] = g_x;
    for (int k = 0; k < 3; ++k) a.out_scale[k] = cfg->in_scale / ZS_SCALE_HOST[k];
    launch_conv(a, 1, st);
    return LPIPS_LAUNCH_STATUS;
}

extern "C" int mrgs_lpips_debug_conv(const MrgsLpipsConvConfig* cfg, const float* in, const float* w, const float* bias, const float* add,
                                     const float* gate, float* out, void* ws, size_t ws_bytes, void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsLpipsConvConfig) || cfg->H < 1 || cfg->W < 1 || (long long)cfg->H * cfg->W > (1ll << 24)) return MRGS_E_BAD_ARG;
    if (!served_pair(cfg->Cin, cfg->Cout) || cfg->n_images < 1 || cfg->n_images > 2) return MRGS_E_BAD_ARG;
    if ((cfg->backward | cfg->relu | cfg->zscore) & ~1) return MRGS_E_BAD_ARG;
    if (!in || !w || !out || !ws || !aligned(in, 16) || !aligned(out, 16) || !aligned(ws, 16) || !aligned(add, 16) || !aligned(gate, 16)) return MRGS_E_BAD_ARG;
    if (ws_bytes < (size_t)36 * cfg->Cin * cfg->Cout) return MRGS_E_BAD_ARG;
    if (cfg->Cin == 3 && (add || gate)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    float* packed = (float*)ws;
    lpips_pack_conv<<<grid_1d((size_t)9 * cfg->Cin * cfg->Cout), 256, 0, st>>>(w, cfg->Cin, cfg->Cout, cfg->backward ? nullptr : packed,
                                                                                cfg->backward ? packed : nullptr);
    ConvArgs a{};
    a.H = cfg->H; a.W = cfg->W; a.relu = cfg->relu; a.w = packed;
    a.Cin = cfg->backward ? cfg->Cout : cfg->Cin;
    a.Cout = cfg->backward ? cfg->Cin : cfg->Cout;
    a.bias = cfg->backward ? nullptr : bias;
    a.zscore = cfg->zscore; a.in_scale = cfg->in_scale; a.in_offset = cfg->in_offset;
    for (int k = 0; k < 3; ++k) a.out_scale[k] = cfg->zscore ? cfg->in_scale / ZS_SCALE_HOST[k] : 1.f;
    const size_t n_in = (size_t)cfg->H * cfg->W * a.Cin, n_out = (size_t)cfg->H * cfg->W * a.Cout;
    for (int k = 0; k < cfg->n_images; ++k) {
        a.in[k] = in + k * n_in; a.out[k] = out + k * n_out;
        a.add[k] = add ? add + k * n_out : nullptr;
        a.gate[k] = gate ? gate + k * n_out : nullptr;
    }
    launch_conv(a, cfg->n_images, st);
    return LPIPS_LAUNCH_STATUS;
}

extern "C" int mrgs_lpips_debug_pool(int32_t H, int32_t W, int32_t C, const float* a, const float* g_pooled, float* out, void* stream)
{
    if (H < 1 || W < 1 || C < 4 || (C & 3) || (long long)H * W > (1ll << 24) || !a || !out || !aligned(a, 16) || !aligned(out, 16)) return MRGS_E_BAD_ARG;
    PoolArgs p{};
    p.H = H; p.W = W; p.C = C; p.a[0] = a; p.out[0] = out; p.g_pooled = g_pooled;
    hipStream_t st = (hipStream_t)stream;
    if (g_pooled) lpips_pool_bwd<<<grid_1d((size_t)H * W * C), 256, 0, st>>>(p);
    else if ((H >> 1) && (W >> 1)) lpips_pool_fwd<<<dim3(grid_1d((size_t)(H >> 1) * (W >> 1) * (C / 4)), 1), 256, 0, st>>>(p);
    return LPIPS_LAUNCH_STATUS;
}

extern "C" int mrgs_lpips_debug_head(int64_t P, int32_t C, const float* fx, const float* fy, const float* w, void* ws, size_t ws_bytes, float* term,
                                     const float* g, float* g_fx, void* stream)
{
    if (P < 1 || P > (1ll << 24) || (C != 64 && C != 128 && C != 256 && C != 512) || !fx || !fy || !w || !ws || !term || !aligned(ws, 16)) return MRGS_E_BAD_ARG;
    if (ws_bytes < (size_t)HEAD_MAX_BLOCKS * HEAD_ROW * sizeof(float) || (g_fx && !g)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    launch_head_fwd(C, fx, fy, w, P, (float*)ws, st);
    HeadFinal fin{};
    fin.first = 0; fin.count = 1; fin.nblocks[0] = head_blocks(P); fin.P[0] = (double)P;
    lpips_head_finalize<<<1, 256, 0, st>>>(fin, (const float*)ws, term);
    if (g_fx) launch_head_bwd(C, fx, fy, w, P, g, 0, g_fx, st);
    return LPIPS_LAUNCH_STATUS;
}
