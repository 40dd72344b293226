// mrgs_model_math.h -- per-gaussian and colour arithmetic shared by the kernel files: each exists here once.
#pragma once
#include "mrgs_internal.h"

// ---- real SH basis, degree <= 3, the 3DGS sign convention (utils/sh_utils.py:57-112, forward.cu:20-81) ----------------------------
// The numbers, once.  The table below has internal linkage: the compiler folds its values into the instructions.  mrgs_preprocess.hip
// declares its own from the same lists with external linkage, as it always has: its kernels LOAD the values, and either linkage given to
// the other side changes the generated code of every kernel that reads the table.
#define MRGS_SH_C0 0.28209479177387814f
#define MRGS_SH_C1 0.4886025119029199f
#define MRGS_SH_C2 {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f}
#define MRGS_SH_C3 {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f, \
                    -0.5900435899266435f}
namespace {
__device__ __constant__ float SH_C0 = MRGS_SH_C0;
__device__ __constant__ float SH_C1 = MRGS_SH_C1;
__device__ __constant__ float SH_C2[5] = MRGS_SH_C2;
__device__ __constant__ float SH_C3[7] = MRGS_SH_C3;
}   // namespace

// basis values of degree 3
__device__ __forceinline__ void sh_basis16(float x, float y, float z, float (&B)[16])
{
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    B[0] = SH_C0;
    B[1] = -SH_C1 * y; B[2] = SH_C1 * z; B[3] = -SH_C1 * x;
    B[4] = SH_C2[0] * xy; B[5] = SH_C2[1] * yz; B[6] = SH_C2[2] * (2.0f * zz - xx - yy); B[7] = SH_C2[3] * xz;
    B[8] = SH_C2[4] * (xx - yy);
    B[9] = SH_C3[0] * y * (3.0f * xx - yy); B[10] = SH_C3[1] * xy * z; B[11] = SH_C3[2] * y * (4.0f * zz - xx - yy);
    B[12] = SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy); B[13] = SH_C3[4] * x * (4.0f * zz - xx - yy);
    B[14] = SH_C3[5] * z * (xx - yy); B[15] = SH_C3[6] * x * (xx - 3.0f * yy);
}

// basis values B[0..n) and their derivatives with respect to the unit direction (x, y, z)
__device__ __forceinline__ void sh_basis_and_grad(int degree, float x, float y, float z, float (&B)[16], float (&Bx)[16], float (&By)[16], float (&Bz)[16])
{
#pragma unroll
    for (int i = 0; i < 16; ++i) { B[i] = 0.f; Bx[i] = 0.f; By[i] = 0.f; Bz[i] = 0.f; }
    B[0] = SH_C0;
    if (degree < 1) return;
    B[1] = -SH_C1 * y; By[1] = -SH_C1;
    B[2] = SH_C1 * z; Bz[2] = SH_C1;
    B[3] = -SH_C1 * x; Bx[3] = -SH_C1;
    if (degree < 2) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    B[4] = SH_C2[0] * xy; Bx[4] = SH_C2[0] * y; By[4] = SH_C2[0] * x;
    B[5] = SH_C2[1] * yz; By[5] = SH_C2[1] * z; Bz[5] = SH_C2[1] * y;
    B[6] = SH_C2[2] * (2.0f * zz - xx - yy); Bx[6] = -2.0f * SH_C2[2] * x; By[6] = -2.0f * SH_C2[2] * y; Bz[6] = 4.0f * SH_C2[2] * z;
    B[7] = SH_C2[3] * xz; Bx[7] = SH_C2[3] * z; Bz[7] = SH_C2[3] * x;
    B[8] = SH_C2[4] * (xx - yy); Bx[8] = 2.0f * SH_C2[4] * x; By[8] = -2.0f * SH_C2[4] * y;
    if (degree < 3) return;
    B[9] = SH_C3[0] * y * (3.0f * xx - yy); Bx[9] = SH_C3[0] * 6.0f * xy; By[9] = SH_C3[0] * 3.0f * (xx - yy);
    B[10] = SH_C3[1] * xy * z; Bx[10] = SH_C3[1] * yz; By[10] = SH_C3[1] * xz; Bz[10] = SH_C3[1] * xy;
    B[11] = SH_C3[2] * y * (4.0f * zz - xx - yy); Bx[11] = -2.0f * SH_C3[2] * xy; By[11] = SH_C3[2] * (4.0f * zz - xx - 3.0f * yy); Bz[11] = 8.0f * SH_C3[2] * yz;
    B[12] = SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy); Bx[12] = -6.0f * SH_C3[3] * xz; By[12] = -6.0f * SH_C3[3] * yz;
    Bz[12] = SH_C3[3] * (6.0f * zz - 3.0f * xx - 3.0f * yy);
    B[13] = SH_C3[4] * x * (4.0f * zz - xx - yy); Bx[13] = SH_C3[4] * (4.0f * zz - 3.0f * xx - yy); By[13] = -2.0f * SH_C3[4] * xy; Bz[13] = 8.0f * SH_C3[4] * xz;
    B[14] = SH_C3[5] * z * (xx - yy); Bx[14] = 2.0f * SH_C3[5] * xz; By[14] = -2.0f * SH_C3[5] * yz; Bz[14] = SH_C3[5] * (xx - yy);
    B[15] = SH_C3[6] * x * (xx - 3.0f * yy); Bx[15] = SH_C3[6] * 3.0f * (xx - yy); By[15] = -6.0f * SH_C3[6] * xy;
}

// IEEE form (the shading kernels keep a v_rcp / v_exp one of their own, sigmoid_fast)
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- wave <-> LDS tile transfer of the [P,15,3] coefficient tensors --------------------------------------------------------------
// 64 consecutive rows of L floats <-> LDS tile, 16 bytes per lane and instruction (the run starts 16-byte aligned because
// the first row index is a multiple of 64); partial waves take the scalar path.  Rows STRIDE floats apart in the tile: odd, so that
// lane-private rows are bank-conflict free
template <int L, int STRIDE = L>
__device__ __forceinline__ void tile_load(float* __restrict__ tile, const float* __restrict__ src, int nrows, int lane)
{
    if (nrows == 64) {
        constexpr int NF4 = 16 * L;
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int k = 0; k * 64 < NF4; k++) {
            const int t = k * 64 + lane;
            if (t < NF4) {
                const float4 v = s4[t];
                const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int e = 4 * t + i;
                    tile[(e / L) * STRIDE + (e % L)] = a[i];
                }
            }
        }
    } else {
        for (int e = lane; e < nrows * L; e += 64) tile[(e / L) * STRIDE + (e % L)] = src[e];
    }
}
template <int L, int STRIDE = L>
__device__ __forceinline__ void tile_store(const float* __restrict__ tile, float* __restrict__ dst, int nrows, int lane)
{
    if (nrows == 64) {
        constexpr int NF4 = 16 * L;
        float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
        for (int k = 0; k * 64 < NF4; k++) {
            const int t = k * 64 + lane;
            if (t < NF4) {
                float a[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int e = 4 * t + i;
                    a[i] = tile[(e / L) * STRIDE + (e % L)];
                }
                d4[t] = make_float4(a[0], a[1], a[2], a[3]);
            }
        }
    } else {
        for (int e = lane; e < nrows * L; e += 64) dst[e] = tile[(e / L) * STRIDE + (e % L)];
    }
}

// ---- the facing normal of a surfel and what hangs on it ---------------------------------------------------------------------------
struct Frame {               // everything the forward derives from (xyz, q, campos) and the backward needs again
    float qlen, qn[4];       // |q|, q / |q| (w, x, y, z)
    float nr[3];             // third column of R(q)
    float flip, nflen, nn[3];// facing sign, |nf|, unit normal
    float dlen, v[3];        // |xyz - campos|, unit view direction
    float c, r[3];           // n . w_o, mirror direction
};

__device__ __forceinline__ Frame make_frame(const float p[3], const float4 q, const float* __restrict__ campos)
{
    Frame f;
    f.qlen = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    f.qn[0] = q.x / f.qlen; f.qn[1] = q.y / f.qlen; f.qn[2] = q.z / f.qlen; f.qn[3] = q.w / f.qlen;
    const float w = f.qn[0], x = f.qn[1], y = f.qn[2], z = f.qn[3];
    f.nr[0] = 2.0f * (x * z + w * y);
    f.nr[1] = 2.0f * (y * z - w * x);
    f.nr[2] = 1.0f - 2.0f * (x * x + y * y);
    const float d[3] = {p[0] - campos[0], p[1] - campos[1], p[2] - campos[2]};
    f.dlen = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    f.v[0] = d[0] / f.dlen; f.v[1] = d[1] / f.dlen; f.v[2] = d[2] / f.dlen;
    const float dotp = -(f.nr[0] * f.v[0] + f.nr[1] * f.v[1] + f.nr[2] * f.v[2]);
    f.flip = dotp >= 0.0f ? 1.0f : -1.0f;
    const float nf[3] = {f.nr[0] * f.flip, f.nr[1] * f.flip, f.nr[2] * f.flip};
    f.nflen = fmaxf(sqrtf(nf[0] * nf[0] + nf[1] * nf[1] + nf[2] * nf[2]), 1e-20f);
    f.nn[0] = nf[0] / f.nflen; f.nn[1] = nf[1] / f.nflen; f.nn[2] = nf[2] / f.nflen;
    f.c = -(f.nn[0] * f.v[0] + f.nn[1] * f.v[1] + f.nn[2] * f.v[2]);       // n . w_o, w_o = -v
    f.r[0] = 2.0f * f.c * f.nn[0] + f.v[0];
    f.r[1] = 2.0f * f.c * f.nn[1] + f.v[1];
    f.r[2] = 2.0f * f.c * f.nn[2] + f.v[2];
    return f;
}

// get_distance (gaussian_renderer/envgs_renderer.py:30-38): normal_cam = n @ Wv[:3,:3], centre_cam = p @ Wv[:3,:3] + Wv[3,:3] with the
// world_view_transform as stored; the distance is |normal_cam . centre_cam|.
struct PlaneDist { float nc[3], cc[3], s; };
__device__ __forceinline__ PlaneDist plane_distance(const float* __restrict__ Wv, const float (&n)[3], const float (&p)[3])
{
    PlaneDist d;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        d.nc[j] = n[0] * Wv[j] + n[1] * Wv[4 + j] + n[2] * Wv[8 + j];
        d.cc[j] = p[0] * Wv[j] + p[1] * Wv[4 + j] + p[2] * Wv[8 + j] + Wv[12 + j];
    }
    d.s = d.nc[0] * d.cc[0] + d.nc[1] * d.cc[1] + d.nc[2] * d.cc[2];
    return d;
}

// Backward of nr = third column of R(qn) (make_frame): d_nr = gradient at nr  ->  d_qn = gradient at the normalised quaternion.
// nr0 = 2 (x z + w y), nr1 = 2 (y z - w x), nr2 = 1 - 2 (x^2 + y^2).  The unit-vector steps before and behind it ((g - n (n . g)) / len)
// stay with the callers: as one function with them the surfel backward comes out with other operand orders, and the callers sum the
// second dot product differently (one in a loop with another, contracted; one un-fused with the association written out).
__device__ __forceinline__ void frame_nr_bwd(const Frame& f, const float (&d_nr)[3], float (&d_qn)[4])
{
    const float w = f.qn[0], x = f.qn[1], y = f.qn[2], z = f.qn[3];
    d_qn[0] = 2.0f * y * d_nr[0] - 2.0f * x * d_nr[1];
    d_qn[1] = 2.0f * z * d_nr[0] - 2.0f * w * d_nr[1] - 4.0f * x * d_nr[2];
    d_qn[2] = 2.0f * w * d_nr[0] + 2.0f * z * d_nr[1] - 4.0f * y * d_nr[2];
    d_qn[3] = 2.0f * x * d_nr[0] + 2.0f * y * d_nr[1];
}

// ---- linear_to_srgb (utils/general_utils) and its derivative -------------------------------------------------------------------------
__device__ __forceinline__ float lin2srgb(float x)
{
    const float eps = 1.1920928955078125e-07f;
    return x <= 0.0031308f ? (323.0f / 25.0f) * x : (211.0f * powf(fmaxf(x, eps), 5.0f / 12.0f) - 11.0f) / 200.0f;
}
__device__ __forceinline__ float lin2srgb_grad(float x)
{
    const float eps = 1.1920928955078125e-07f;
    if (x <= 0.0031308f) return 323.0f / 25.0f;
    return x >= eps ? (211.0f / 200.0f) * (5.0f / 12.0f) * powf(x, -7.0f / 12.0f) : 0.0f;
}
