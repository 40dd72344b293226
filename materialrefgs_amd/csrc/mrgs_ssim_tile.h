// mrgs_ssim_tile.h -- the 11x11 Gaussian window moments of one 32x32 pixel tile, stated once for the two kernels that need them: the fused
// training loss (mrgs_loss.hip: loss_fwd_kernel) and the evaluation metrics (mrgs_eval.hip: eval_metrics_kernel).
//
// ssim / _ssim / create_window (utils/loss_utils.py:83-119): both images of a tile staged with a 5-pixel halo in LDS, the five window moments
// (mu1, mu2, E[x^2], E[y^2], E[xy]) by a separable pass, rows then columns, four outputs per thread from a sliding window.  Zero padding as
// F.conv2d(padding=5): pixels outside the image count as 0.  The one difference between the callers is a compile-time one: the evaluation
// clamps both images to [0, 1] as they are read (eval.py:44-46), the loss takes them as they are -- no branch per caller at run time, and the
// loss kernel's instructions are the ones it had before this header existed.
#pragma once
#include <math.h>

constexpr int LT = 32;            // tile edge
constexpr int LP = 4;             // outputs per thread and pass (256 threads x 4 = 32 x 32)
constexpr int LR = 5;             // window radius (window_size 11, loss_utils.py:91)
constexpr int LH = LT + 2 * LR;   // tile + halo

// gaussian(11, 1.5) (loss_utils.py:28-30): exp in double, stored as fp32, divided by their fp32 sum (torch's sum of these 11
// values equals the correctly rounded one; tests/golden/reference_loss.npz holds the resulting window)
static inline void ssim_window(float w[2 * LR + 1])
{
    float g[2 * LR + 1];
    double sum = 0.0;
    for (int i = 0; i <= 2 * LR; ++i) {
        const double d = (double)(i - LR);
        g[i] = (float)exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += (double)g[i];
    }
    for (int i = 0; i <= 2 * LR; ++i) w[i] = g[i] / (float)sum;
}

// tile (bx, by) of the planes I1, I2 [H, W] into s1, s2 with the halo; CLAMP: values clamped to [0, 1] on the way (a NaN stays a NaN)
template <bool CLAMP>
__device__ __forceinline__ void ssim_tile_stage(const float* __restrict__ I1, const float* __restrict__ I2, int H, int W, int bx, int by, int tid,
                                                float (&s1)[LH][LH + 1], float (&s2)[LH][LH + 1])
{   // all loads of the tile in flight before the first LDS store (a rolled loop waits for every round trip in turn)
    constexpr int NL = (LH * LH + 255) / 256;
    float v1[NL], v2[NL];
#pragma unroll
    for (int n = 0; n < NL; ++n) {
        const int i = tid + n * 256, r = i / LH, cc = i - r * LH, y = by + r - LR, x = bx + cc - LR;
        const bool in = (i < LH * LH) & (x >= 0) & (x < W) & (y >= 0) & (y < H);
        v1[n] = in ? I1[(size_t)y * W + x] : 0.f;
        v2[n] = in ? I2[(size_t)y * W + x] : 0.f;
        if (CLAMP) {                                                  // torch.clamp(x, 0, 1): min(max(x, 0), 1) with NaN passed on
            v1[n] = v1[n] < 0.f ? 0.f : (v1[n] > 1.f ? 1.f : v1[n]);
            v2[n] = v2[n] < 0.f ? 0.f : (v2[n] > 1.f ? 1.f : v2[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < NL; ++n) {
        const int i = tid + n * 256, r = i / LH, cc = i - r * LH;
        if (i < LH * LH) { s1[r][cc] = v1[n]; s2[r][cc] = v2[n]; }
    }
}

// rows: a thread produces LP consecutive outputs of one row from LP + 10 inputs (sliding window: 3.1 LDS reads per output
// and quantity instead of 11)
__device__ __forceinline__ void ssim_tile_rows(const float (&w11)[2 * LR + 1], int tid, const float (&s1)[LH][LH + 1], const float (&s2)[LH][LH + 1],
                                               float (&hz)[5][LH][LT + 1])
{
#pragma unroll 2
    for (int it = tid; it < LH * (LT / LP); it += 256) {
        const int r = it / (LT / LP), c0 = (it - r * (LT / LP)) * LP;
        float p[LP + 2 * LR], q[LP + 2 * LR];
#pragma unroll
        for (int j = 0; j < LP + 2 * LR; ++j) { p[j] = s1[r][c0 + j]; q[j] = s2[r][c0 + j]; }
#pragma unroll
        for (int o = 0; o < LP; ++o) {
            float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * LR; ++k) {
                const float w = w11[k], wp = w * p[o + k], wq = w * q[o + k];
                m1 += wp; m2 += wq; e11 = fmaf(wp, p[o + k], e11); e22 = fmaf(wq, q[o + k], e22); e12 = fmaf(wp, q[o + k], e12);
            }
            hz[0][r][c0 + o] = m1; hz[1][r][c0 + o] = m2; hz[2][r][c0 + o] = e11; hz[3][r][c0 + o] = e22; hz[4][r][c0 + o] = e12;
        }
    }
}

// columns: thread (tx, tg) produces the LP outputs (tx, LP tg .. LP tg + LP - 1) of the five moments
__device__ __forceinline__ void ssim_tile_cols(const float (&w11)[2 * LR + 1], int tx, int y0, const float (&hz)[5][LH][LT + 1], float (&mom)[5][LP])
{
#pragma unroll
    for (int qn = 0; qn < 5; ++qn) {
        float v[LP + 2 * LR];
#pragma unroll
        for (int j = 0; j < LP + 2 * LR; ++j) v[j] = hz[qn][y0 + j][tx];
#pragma unroll
        for (int o = 0; o < LP; ++o) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * LR; ++k) acc = fmaf(w11[k], v[o + k], acc);
            mom[qn][o] = acc;
        }
    }
}

// the SSIM value of one pixel from its five moments (loss_utils.py:103-110) with the four factors the loss's derivative maps are made of
struct SsimPoint { float S, A1, A2, B1, B2, inv; };
__device__ __forceinline__ SsimPoint ssim_point(float mu1, float mu2, float e11, float e22, float e12)
{
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;            // loss_utils.py:107-108
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const float sg1 = e11 - mu1_sq, sg2 = e22 - mu2_sq, sg12 = e12 - mu12;
    SsimPoint p;
    p.A1 = 2.f * mu12 + C1; p.A2 = 2.f * sg12 + C2; p.B1 = mu1_sq + mu2_sq + C1; p.B2 = sg1 + sg2 + C2;
    p.inv = 1.f / (p.B1 * p.B2);
    p.S = p.A1 * p.A2 * p.inv;                                      // :110
    return p;
}
