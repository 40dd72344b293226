// mrgs_rgb8.h -- what the two files that turn maps into 8-bit RGB share (mrgs_eval.hip: mrgs_export_rgb8; mrgs_sheet.hip: mrgs_sheet_rgb8):
// the colour table, the byte rule, the per-workgroup minimum / maximum of a map with its fold, and the store of a run of LDS bytes as whole
// dwords.  Each exists here once.
#pragma once
#include "mrgs_internal.h"
#include "mrgs_wave.h"

namespace {

// ---- the colour table of the jet-coloured maps ---------------------------------------------------------------------------------------
// THIS LIBRARY'S OWN jet, parity with cv2's COLORMAP_JET table unpinned (cv2 is not installed where this is built, so its array can be
// neither read nor pinned).  For level L, v = L / 255 in double:
//   r = clamp(1.5 - |4 v - 3|, 0, 1), g = clamp(1.5 - |4 v - 2|, 0, 1), b = clamp(1.5 - |4 v - 1|, 0, 1), byte = floor(255 c + 0.5)
// evaluated by the compiler (IEEE double, nothing fused), the same 768 bytes for the device and for mrgs_eval_jet_table.  Which pixel gets
// which row -- the level -- is what is pinned to the reference's statement.
struct JetTable { uint8_t rgb[256][3]; };
constexpr uint8_t jet_byte(double v, double k)
{
    double d = 4.0 * v - k;
    if (d < 0.0) d = -d;
    double c = 1.5 - d;
    c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
    return (uint8_t)(int)(255.0 * c + 0.5);                          // floor of a value >= 0
}
constexpr JetTable make_jet()
{
    JetTable t{};
    for (int L = 0; L < 256; ++L) {
        const double v = (double)L / 255.0;
        t.rgb[L][0] = jet_byte(v, 3.0); t.rgb[L][1] = jet_byte(v, 2.0); t.rgb[L][2] = jet_byte(v, 1.0);
    }
    return t;
}
constexpr JetTable JET = make_jet();
__constant__ JetTable d_jet = make_jet();                            // one copy per file that includes this header (768 bytes)

constexpr int XCHUNK = 1024;      // pixels per workgroup of the byte kernels: 256 threads x 4

// trunc(clamp(v, 0, 255)) as a byte; NaN -> 0
__device__ __forceinline__ uint32_t to_byte(float v) { return v >= 0.f ? (uint32_t)(int)fminf(v, 255.f) : 0u; }

// torchvision's x.mul(255).add_(0.5).clamp_(0, 255).to(uint8): the product and the sum rounded separately
__device__ __forceinline__ uint32_t unit_byte(float x) { return to_byte(__fadd_rn(__fmul_rn(x, 255.f), 0.5f)); }

// ---- minimum and maximum of a map -------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads, NaN skipped (fminf / fmaxf); exact in any order.  red: 8 floats of LDS.  The result is valid in thread 0.
__device__ __forceinline__ float2 block_minmax(float mn, float mx, int tid, float (*red)[2])
{
    mn = wave_shfl_min(mn); mx = wave_shfl_max(mx);
    if ((tid & 63) == 0) { red[tid >> 6][0] = mn; red[tid >> 6][1] = mx; }
    __syncthreads();
    return make_float2(fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0])),
                       fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1])));
}

// ---- a run of LDS bytes to global memory ---------------------------------------------------------------------------------------------------
// global bytes [obase, obase + nbytes) of `out` (4-byte aligned) = LDS bytes [shift, shift + nbytes) of `sb`, shift = obase & 3, so that a
// 4-byte aligned global address is a 4-byte aligned LDS offset: bytes up to the first aligned dword, whole dwords, bytes behind.  Called by
// all 256 threads behind the barrier that ends the writes to sb.
__device__ __forceinline__ void store_lds_bytes(const uint8_t* sb, int shift, int nbytes, uint8_t* __restrict__ out, size_t obase, int tid)
{
    const int end = shift + nbytes;
    const int body0 = shift ? 4 : 0, body1 = end & ~3;                              // LDS offsets of the dword body [body0, body1)
    uint8_t* __restrict__ o = out + (obase - shift);                                // 4-byte aligned (out is)
    if (body1 > body0) {
        for (int w = body0 / 4 + tid; w < body1 / 4; w += 256)
            reinterpret_cast<uint32_t*>(o)[w] = reinterpret_cast<const uint32_t*>(sb)[w];
        if (tid < body0 - shift && shift) o[shift + tid] = sb[shift + tid];
        if (tid < end - body1) o[body1 + tid] = sb[body1 + tid];
    } else {                                                                        // fewer bytes than reach an aligned dword
        for (int i = shift + tid; i < end; i += 256) o[i] = sb[i];
    }
}

}   // namespace
