// mrgs_prefilter.hip -- the environment prefilter (EnvLight.build_mips, scene/light.py:72-86) on gfx950.
//
//   cubemap_filter_build_kernel<>  the GGX / cosine filter of one level as a sparse matrix (count pass, fill pass)
//   csr_spmv3*_kernel              that matrix times a 3-channel cubemap: plain CSR, blocked rows, and the batched launch of all levels
//                                  with the rows of one fundamental domain of the cube's 48 symmetries as a matrix product on the MFMA pipe
//   cubemap_mip_*_kernel           the 2x2 box mip chain and the reference's backward of it
// each group followed by its entry points; MRGS_SPMV_TRACE is the developer hook of the batched launch.
//
// The reference runs, every iteration, renderutils' specular_cubemap on each mip level (scene/renderutils/c_src/
// cubemap.cu:238-354: per output texel a loop over a bounds window with GGX weights, backward = the same loop with three
// atomics per (texel, window texel) pair) and diffuse_cubemap on the last one (:110-166).  For a given (resolution,
// roughness, cutoff) those filters are FIXED linear operators on the cubemap: out[t] = sum_s w(t, s) cube[s] / sum_s w(t, s).
// Here the operator is materialised once as a sparse matrix (CSR, normalised weights; a second CSR holds its transpose) and
// every iteration is a 3-channel SpMV each way -- no transcendental per pair, no atomics, deterministic, and bound by
// streaming 8 bytes per non-zero from HBM (26 M non-zeros for the 128/64/32/16 chain of the reference's defaults).
// Cube addressing (f3, face_to_dir, dir_to_face, cube_taps) comes from mrgs_envmap.h; the weights restate the reference's operation for
// operation and keep the IEEE quotient.
#include "mrgs_envmap.h"

// ---- the filters as sparse matrices ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cm_pixel_area(int x, int y, int N)
{   // cubemap.cu:17-30
    if (N <= 1) return 1.0f;
    const int H = N / 2;
    x = abs(x - H); y = abs(y - H);
    const float dx = atanf((float)(x + 1) / (float)H) - atanf((float)x / (float)H);
    const float dy = atanf((float)(y + 1) / (float)H) - atanf((float)y / (float)H);
    return dx * dy;
}
__device__ __forceinline__ f3 cm_normalize(f3 v)
{   // safeNormalize of renderutils (vec3f.h): v / sqrt(max(dot, tiny))
    const float l = sqrtf(fmaxf(dot3(v, v), 1e-20f));
    return mk(v.x / l, v.y / l, v.z / l);
}
__device__ __forceinline__ f3 cm_cube_to_dir(int x, int y, int side, int N)
{   // cubemap.cu:32-46 (same face convention as face_to_dir)
    const float fx = 2.0f * (((float)x + 0.5f) / (float)N) - 1.0f;
    const float fy = 2.0f * (((float)y + 0.5f) / (float)N) - 1.0f;
    return cm_normalize(face_to_dir(side, fx, fy));
}
__device__ __forceinline__ float cm_ndf_ggx(float alphaSqr, float cosTheta)
{   // cubemap.cu:171-176
    const float c = fminf(fmaxf(cosTheta, 0.0f), 1.0f);
    const float d = (c * alphaSqr - c) * c + 1.0f;
    return alphaSqr / (d * d * 3.14159265358979323846f);
}
// weight of source texel (x, y, s) for the output direction VNR; <= 0 when the texel does not take part
__device__ __forceinline__ float cm_weight(int kind, f3 VNR, int x, int y, int s, int N, float alphaSqr, float cos_cutoff, bool& take)
{
    const f3 L = cm_cube_to_dir(x, y, s, N);
    const float d = dot3(L, VNR);
    if (kind == 0) {   // specular (cubemap.cu:262-276)
        take = d >= cos_cutoff;
        if (!take) return 0.0f;
        const f3 Hh = cm_normalize(mk(L.x + VNR.x, L.y + VNR.y, L.z + VNR.z));
        const float wiDotN = fmaxf(d, 0.0f), vh = fmaxf(dot3(VNR, Hh), 0.0f);
        return wiDotN * cm_ndf_ggx(alphaSqr, vh) * cm_pixel_area(x, y, N) / 4.0f;
    }
    take = true;       // diffuse (cubemap.cu:124-136): every texel, cosine clamped to [0, 0.999]
    const float ct = fminf(fmaxf(d, 0.0f), 0.999f);
    return ct * cm_pixel_area(x, y, N) / 3.141592f;
}

// pass 0: count the non-zeros of each row and sum its weights; pass 1: write column indices and normalised weights.
// One thread per output texel; 16x16 source tiles are culled with the interval test of SpecularBoundsKernel (cubemap.cu:203-214).
template <int PASS>
__global__ void __launch_bounds__(256) cubemap_filter_build_kernel(int N, int kind, float roughness, float cos_cutoff, uint32_t* __restrict__ row_count,
                                                                   float* __restrict__ row_wsum, const uint32_t* __restrict__ row_ptr,
                                                                   uint32_t* __restrict__ col, float* __restrict__ val)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int NT = 6 * N * N;
    if (t >= NT) return;
    const int px = t % N, py = (t / N) % N, pz = t / (N * N);
    const f3 VNR = cm_cube_to_dir(px, py, pz, N);
    const float alpha = roughness * roughness, alphaSqr = alpha * alpha;
    uint32_t cnt = 0;
    float wsum = 0.0f;
    uint32_t at = PASS == 1 ? row_ptr[t] : 0u;
    const float inv = PASS == 1 ? (kind == 0 ? 1.0f / row_wsum[t] : 1.0f) : 0.0f;   // only specular_cubemap divides by the weight sum (ops.py:459)
    const int TS = 16;
    for (int s = 0; s < 6; s++)
        for (int ty = 0; ty < (N + TS - 1) / TS; ty++)
            for (int tx = 0; tx < (N + TS - 1) / TS; tx++) {
                const int tsx = tx * TS, tsy = ty * TS, tex = min((tx + 1) * TS, N), tey = min((ty + 1) * TS, N);
                if (kind == 0) {
                    const f3 L0 = cm_cube_to_dir(tsx, tsy, s, N), L1 = cm_cube_to_dir(tex, tsy, s, N);
                    const f3 L2 = cm_cube_to_dir(tsx, tey, s, N), L3 = cm_cube_to_dir(tex, tey, s, N);
                    const float minx = fminf(fminf(L0.x, L1.x), fminf(L2.x, L3.x)), maxx = fmaxf(fmaxf(L0.x, L1.x), fmaxf(L2.x, L3.x));
                    const float miny = fminf(fminf(L0.y, L1.y), fminf(L2.y, L3.y)), maxy = fmaxf(fmaxf(L0.y, L1.y), fmaxf(L2.y, L3.y));
                    const float minz = fminf(fminf(L0.z, L1.z), fminf(L2.z, L3.z)), maxz = fmaxf(fmaxf(L0.z, L1.z), fmaxf(L2.z, L3.z));
                    const float maxdp = fmaxf(minx * VNR.x, maxx * VNR.x) + fmaxf(miny * VNR.y, maxy * VNR.y) + fmaxf(minz * VNR.z, maxz * VNR.z);
                    if (maxdp < cos_cutoff) continue;
                }
                for (int y = tsy; y < tey; y++)
                    for (int x = tsx; x < tex; x++) {
                        bool take;
                        const float w = cm_weight(kind, VNR, x, y, s, N, alphaSqr, cos_cutoff, take);
                        if (!take) continue;
                        if (PASS == 0) { cnt++; wsum += w; }
                        else { col[at] = (uint32_t)((s * N + y) * N + x); val[at] = w * inv; at++; }
                    }
            }
    if (PASS == 0) { row_count[t] = cnt; row_wsum[t] = wsum; }
}

// entry points of the filter build
extern "C" {

int mrgs_cubemap_filter_count(int32_t res, int32_t kind, float roughness, float cos_cutoff, uint32_t* row_count, float* row_wsum, void* stream)
{
    if (res < 1 || res > 1024 || (kind != 0 && kind != 1) || !row_count || !row_wsum) return MRGS_E_BAD_ARG;
    const int NT = 6 * res * res;
    hipLaunchKernelGGL(cubemap_filter_build_kernel<0>, dim3((NT + 255) / 256), dim3(256), 0, (hipStream_t)stream, res, kind, roughness, cos_cutoff,
                       row_count, row_wsum, (const uint32_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
    return MRGS_LAUNCH_STATUS();
}

int mrgs_cubemap_filter_fill(int32_t res, int32_t kind, float roughness, float cos_cutoff, const uint32_t* row_ptr, const float* row_wsum,
                             uint32_t* col, float* val, void* stream)
{
    if (res < 1 || res > 1024 || (kind != 0 && kind != 1) || !row_ptr || !row_wsum || !col || !val) return MRGS_E_BAD_ARG;
    const int NT = 6 * res * res;
    hipLaunchKernelGGL(cubemap_filter_build_kernel<1>, dim3((NT + 255) / 256), dim3(256), 0, (hipStream_t)stream, res, kind, roughness, cos_cutoff,
                       (uint32_t*)nullptr, const_cast<float*>(row_wsum), row_ptr, col, val);
    return MRGS_LAUNCH_STATUS();
}

}   // extern "C"

// ---- the products: a filter matrix times a 3-channel cubemap ---------------------------------------------------------------------------
// y[r, 0..2] = sum_k val[k] x[col[k], 0..2] over the non-zeros of row r; G lanes per row (4: short rows, 64: long rows).
// The kernel streams its matrix from HBM once per call, so the matrix is kept small: 16-bit column indices when they fit and
// 16-bit fixed-point weights with one fp32 scale per row (weight = q * scale[r], q in [0, 65535]: absolute error <= row
// maximum / 131070 per weight, ~1e-6 of the result for the rows of hundreds of similar weights these filters have).
#ifndef MRGS_SPMV_ROUNDS
#define MRGS_SPMV_ROUNDS 4
#endif
template <int G, typename IDX, typename WT>
__device__ __forceinline__ void csr_spmv3_body(int block, int nrows, const uint32_t* __restrict__ row_ptr, const IDX* __restrict__ col,
                                               const WT* __restrict__ val, const float* __restrict__ row_scale, const float* __restrict__ x,
                                               float* __restrict__ y)
{
    const int gid = (block * 256 + threadIdx.x) / G, sub = threadIdx.x % G;
    const int r = min(gid, nrows - 1);
    const uint32_t a = row_ptr[r], b = gid < nrows ? row_ptr[r + 1] : a;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t k = a + sub;
    // The matrix streams from HBM (it does not survive in the last-level cache between two iterations of a training step) and a wave
    // has only 2 x 128 bytes of it in flight per round: with every wave slot of the chip taken that is 2 MB against the ~8 MB that
    // 8 TB/s x 1 us of latency want.  MRGS_SPMV_ROUNDS rounds of (index, weight) loads are issued before the first gather.
    for (; k + (MRGS_SPMV_ROUNDS - 1) * G < b; k += MRGS_SPMV_ROUNDS * G) {
        uint32_t c[MRGS_SPMV_ROUNDS];
        float w[MRGS_SPMV_ROUNDS], v[MRGS_SPMV_ROUNDS][3];
#pragma unroll
        for (int u = 0; u < MRGS_SPMV_ROUNDS; ++u) { c[u] = col[k + u * G]; w[u] = (float)val[k + u * G]; }
#pragma unroll
        for (int u = 0; u < MRGS_SPMV_ROUNDS; ++u) {
            const float* xv = x + 3 * (size_t)c[u];
            v[u][0] = xv[0]; v[u][1] = xv[1]; v[u][2] = xv[2];
        }
#pragma unroll
        for (int u = 0; u < MRGS_SPMV_ROUNDS; ++u) { s0 += w[u] * v[u][0]; s1 += w[u] * v[u][1]; s2 += w[u] * v[u][2]; }
    }
    for (; k < b; k += G) {
        const float w = (float)val[k];
        const float* xv = x + 3 * (size_t)col[k];
        s0 += w * xv[0]; s1 += w * xv[1]; s2 += w * xv[2];
    }
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) {
        s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64);
    }
    if (sub == 0 && gid < nrows) {
        const float sc = row_scale != nullptr ? row_scale[r] : 1.0f;
        y[3 * (size_t)r] = s0 * sc; y[3 * (size_t)r + 1] = s1 * sc; y[3 * (size_t)r + 2] = s2 * sc;
    }
}

// Blocked rows ("val_bytes == 8"): the long rows of the GGX / cosine filters touch runs of ~10-17 consecutive texels, so a row is stored
// as blocks of four consecutive columns -- a 16-bit block index (column / 4) and four 16-bit fixed-point weights (zero where the row has
// no entry; 0.88-0.93 of the slots are used) = 2.8 bytes per non-zero instead of 4, and ONE 48-byte gather of x (three 16-byte loads,
// 4 texels x 3 channels) instead of four gathers of 12 bytes.  64 lanes per row, one block per lane and round.  row_ptr counts blocks.
#ifndef MRGS_SPMV_BLK_ROUNDS
#define MRGS_SPMV_BLK_ROUNDS 2      // measured in the batched prefilter launch: 2 rounds 43.5 us, 4 rounds 51.5 (66 VGPRs), 8 rounds 47.7; plain CSR 51.4
#endif
// (Also measured: a wave owning 2 / 4 / 8 consecutive rows and walking their blocks as one range, products added to the row's accumulators
// with 0/1 factors -- fewer, longer waves without the partly empty last round per row: 45.7 / 54.6 / 74.7 us against 42.6 for a row per
// wave.  Round 4: a wave owning 2 / 4 / 8 rows strided by the wave count, software-pipelined ACROSS rows -- the next row's extent fetched
// two rows ahead, its first round of (index, weights) one row ahead, so that a row starts with its gathers instead of three dependent
// round trips: the same time at 2 rows, +5 us (forward) and +15 us (transposed call) at 4, +16 us (forward) at 8, bit-identical sums.  The launch wants MANY short waves;
// what holds it at 1.7 TB/s was not found.)
__device__ __forceinline__ void csr_spmv3_blk4_body(int block, int nrows, const uint32_t* __restrict__ row_ptr, const uint16_t* __restrict__ bcol,
                                                    const uint2* __restrict__ bval, const float* __restrict__ row_scale,
                                                    const float* __restrict__ x, float* __restrict__ y)
{
    const int gid = (block * 256 + threadIdx.x) / 64, sub = threadIdx.x % 64;
    const int r = min(gid, nrows - 1);
    const uint32_t a = row_ptr[r], b = gid < nrows ? row_ptr[r + 1] : a;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    auto consume = [&](uint32_t c, uint2 w, const float4& v0, const float4& v1, const float4& v2) {
        const float w0 = (float)(w.x & 0xFFFFu), w1 = (float)(w.x >> 16), w2 = (float)(w.y & 0xFFFFu), w3 = (float)(w.y >> 16);
        s0 = fmaf(w0, v0.x, s0); s1 = fmaf(w0, v0.y, s1); s2 = fmaf(w0, v0.z, s2);
        s0 = fmaf(w1, v0.w, s0); s1 = fmaf(w1, v1.x, s1); s2 = fmaf(w1, v1.y, s2);
        s0 = fmaf(w2, v1.z, s0); s1 = fmaf(w2, v1.w, s1); s2 = fmaf(w2, v2.x, s2);
        s0 = fmaf(w3, v2.y, s0); s1 = fmaf(w3, v2.z, s1); s2 = fmaf(w3, v2.w, s2);
    };
    uint32_t k = a + sub;
    // MRGS_SPMV_BLK_ROUNDS rounds in flight: a wave has only 64 x 10 bytes of the matrix per round, and the gather of x depends on it
    for (; k + (MRGS_SPMV_BLK_ROUNDS - 1) * 64 < b; k += MRGS_SPMV_BLK_ROUNDS * 64) {
        uint32_t c[MRGS_SPMV_BLK_ROUNDS];
        uint2 w[MRGS_SPMV_BLK_ROUNDS];
        float4 v[MRGS_SPMV_BLK_ROUNDS][3];
#pragma unroll
        for (int u = 0; u < MRGS_SPMV_BLK_ROUNDS; ++u) { c[u] = bcol[k + u * 64]; w[u] = bval[k + u * 64]; }
#pragma unroll
        for (int u = 0; u < MRGS_SPMV_BLK_ROUNDS; ++u) {
            const float4* p = reinterpret_cast<const float4*>(x) + 3 * (size_t)c[u];
            v[u][0] = p[0]; v[u][1] = p[1]; v[u][2] = p[2];
        }
#pragma unroll
        for (int u = 0; u < MRGS_SPMV_BLK_ROUNDS; ++u) consume(c[u], w[u], v[u][0], v[u][1], v[u][2]);
    }
    for (; k < b; k += 64) {
        const uint32_t c0 = bcol[k];
        const uint2 w0 = bval[k];
        const float4* p0 = reinterpret_cast<const float4*>(x) + 3 * (size_t)c0;
        const float4 a0 = p0[0], a1 = p0[1], a2 = p0[2];
        consume(c0, w0, a0, a1, a2);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64);
    }
    if (sub == 0 && gid < nrows) {
        const float sc = row_scale[r];
        y[3 * (size_t)r] = s0 * sc; y[3 * (size_t)r + 1] = s1 * sc; y[3 * (size_t)r + 2] = s2 * sc;
    }
}
__global__ void __launch_bounds__(256) csr_spmv3_blk4_kernel(int nrows, const uint32_t* __restrict__ row_ptr, const uint16_t* __restrict__ bcol,
                                                             const uint2* __restrict__ bval, const float* __restrict__ row_scale,
                                                             const float* __restrict__ x, float* __restrict__ y)
{
    csr_spmv3_blk4_body((int)blockIdx.x, nrows, row_ptr, bcol, bval, row_scale, x, y);
}

template <int G, typename IDX, typename WT>
__global__ void __launch_bounds__(256) csr_spmv3_kernel(int nrows, const uint32_t* __restrict__ row_ptr, const IDX* __restrict__ col,
                                                        const WT* __restrict__ val, const float* __restrict__ row_scale,
                                                        const float* __restrict__ x, float* __restrict__ y)
{
    csr_spmv3_body<G, IDX, WT>((int)blockIdx.x, nrows, row_ptr, col, val, row_scale, x, y);
}

// (Tried in round 3 and removed: the long-row levels with their vector resident in LDS -- 16 x 16 / 32 x 32 cubemaps whole, a 64 x 64 face
// as one of six panels, 16 bytes per texel, a workgroup per block of rows walking the panels its rows touch.  Correct, and 80-150 us per
// call against 50 us for the streaming kernel below: one 1 024-thread workgroup per CU (or two of 512) in lock step through
// stage / barrier / consume phases keeps fewer requests in flight than 2 500 independent 256-thread workgroups do, whatever the gathers cost.)
// Several independent SpMVs in ONE launch (the levels of the environment prefilter: four launches of 9-18 us each were mostly the
// latency of streaming each matrix with a fraction of the chip; together the matrices stream with every wave slot busy).  A workgroup
// finds its product from a table in the kernel arguments (wave-uniform scan) and runs the body of its storage format.
struct SpmvSeg {
    int nrows, fmt, first_block, log2n;
    const uint32_t* row_ptr; const void* col; const void* val; const float* row_scale; const float* x; float* y;
    // format 16 (tiles of rows of ONE fundamental domain of the cube's symmetry group, below): the row -> image rows table, the factor of
    // the vector's texels, the tiles' row ranges, their panels (the column blocks a tile's rows touch); `val` = the tiles' dense weights
    const int32_t* image_rows; const float* pre; const uint32_t* tile_ptr; const uint32_t* panel_ptr; const uint16_t* panel_src;
};
struct SpmvBatch { int n; int total_blocks; uint64_t sym[48]; SpmvSeg seg[MRGS_SPMV_MAX_BATCH]; unsigned long long* trace; };

// ---- the filters as operators on ONE fundamental domain of the cube's 48 symmetries -------------------------------------------------
// A filter weight is K(r, c) * area(c) / n(r): K (GGX lobe x cosine x cut-off x the reference's tile cull) depends on the two directions
// only and is invariant under the 48 signed axis permutations g, which map the texel grid of a cube map onto itself:
// K(g r, g c) = K(r, c).  (The solid angle `area` of the reference, cubemap.cu:17-30, is NOT invariant -- it is off by one texel on the
// negative half of a face -- and the row sum n inherits that; both are per-texel factors and stay outside.)  So
//     y[g r0] = post[g r0] * sum_c K'(r0, c) * (pre * x)[g c]
// for the N/2 (N/2 + 1) / 2 rows r0 of a triangle of face 0: the matrix is 1/47 of the full one (60 MB -> 1.3 MB for the 64 x 64 level)
// and stays in the L2 of every XCD instead of streaming from HBM each call and each way.  That alone bought little: with its matrix
// cached the gather kernel is bound by the gather of x itself (48 bytes per block of four columns, 350 MB a call: 33 us against 43 from
// HBM), and with x staged in LDS per (tile of rows, symmetry) by the instructions of 64-lane reductions per row (measured, round 5).
// What the symmetry really gives is a matrix PRODUCT: the rows of a 4 x 4 TILE of the triangle touch the same ~1 000-2 300 texels (the
// tile's PANEL, 60 % of it per row), so a tile is a dense 16 x K matrix, and the 48 symmetries x 3 channels are 144 right-hand sides:
//     Y[16 rows][48 g x 3] = W[16][K] * X[K][48 g x 3],   X[k][g, :] = (pre * x)[g panel_k]
// on v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: an fmaf chain; the 16-bit fixed-point weights are exact in f32).  A workgroup =
// (tile, four symmetries: 16 columns with the channel padded to four); its four waves split K; a wave stages 16 texels x 4 symmetries
// per step (one (texel, symmetry) per lane: 12 bytes of x and its factor -> 16 bytes of LDS, wave-private, double-buffered) for four MFMAs.
// sym[g] packs, per SOURCE face s (6 bits each): image face | axes exchanged << 3 | row flipped << 4 | column flipped << 5.
struct CubeImage { int s, y, x; };
static inline CubeImage cube_symmetry_image(int g, int N, int s, int y, int x)
{
    static const int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int u = 2 * x - (N - 1), v = 2 * y - (N - 1);       // texel centre in units of 1 / N, the major axis at +-N (face_to_dir)
    int d[3];
    switch (s) {
    case 0: d[0] = N; d[1] = -v; d[2] = -u; break;
    case 1: d[0] = -N; d[1] = -v; d[2] = u; break;
    case 2: d[0] = u; d[1] = N; d[2] = v; break;
    case 3: d[0] = u; d[1] = -N; d[2] = -v; break;
    case 4: d[0] = u; d[1] = -v; d[2] = N; break;
    default: d[0] = -u; d[1] = -v; d[2] = -N; break;
    }
    int e[3];
    for (int i = 0; i < 3; ++i) e[i] = (((g & 7) >> i) & 1) ? -d[PERM[g >> 3][i]] : d[PERM[g >> 3][i]];
    int uu, vv, ss;
    if (e[0] == N) { ss = 0; vv = -e[1]; uu = -e[2]; }
    else if (e[0] == -N) { ss = 1; vv = -e[1]; uu = e[2]; }
    else if (e[1] == N) { ss = 2; uu = e[0]; vv = e[2]; }
    else if (e[1] == -N) { ss = 3; uu = e[0]; vv = -e[2]; }
    else if (e[2] == N) { ss = 4; uu = e[0]; vv = -e[1]; }
    else { ss = 5; uu = -e[0]; vv = -e[1]; }
    return {ss, (vv + N - 1) / 2, (uu + N - 1) / 2};
}
static void cube_symmetry_table(uint64_t* tab)
{
    for (int g = 0; g < 48; ++g) {
        uint64_t t = 0;
        for (int s = 0; s < 6; ++s) {
            const CubeImage o = cube_symmetry_image(g, 4, s, 0, 0), ax = cube_symmetry_image(g, 4, s, 0, 1), ay = cube_symmetry_image(g, 4, s, 1, 0);
            const bool swap = ax.x == o.x;                       // a step along x moves the image along y
            const bool fc = swap ? ax.y < o.y : ax.x < o.x;      // the image runs backwards along the source's x
            const bool fr = swap ? ay.x < o.x : ay.y < o.y;      // ... along the source's y
            t |= (uint64_t)(o.s | (swap ? 8 : 0) | (fr ? 16 : 0) | (fc ? 32 : 0)) << (6 * s);
        }
        tab[g] = t;
    }
}

#ifndef MRGS_SPMV_BATCH_THREADS
#define MRGS_SPMV_BATCH_THREADS 512
#endif
#define MRGS_SPMV_SYM_WAVES (MRGS_SPMV_BATCH_THREADS / 64)      // the waves of a workgroup split the panel
static_assert(128 * MRGS_SPMV_SYM_WAVES >= MRGS_SPMV_MAX_PANEL, "a wave holds the patch ids of 128 steps");
#define MRGS_SPMV_SYM_BROW 20        // floats per staged texel row: 16 columns + 4 of padding (the 16-byte writes of eight lanes then cover the 32 banks)
#define MRGS_SPMV_SYM_LDS (MRGS_SPMV_SYM_WAVES * (16 * MRGS_SPMV_SYM_BROW * 4 + 1024))  // per wave: a staging buffer of 16 texels x 16 columns, a partial tile
#ifndef MRGS_SPMV_SYM_DEPTH
#define MRGS_SPMV_SYM_DEPTH 2       // steps of gathers in flight ahead of the MFMAs (a step waits for nothing younger than DEPTH steps)
#endif
typedef float spmv_f32x4 __attribute__((ext_vector_type(4)));
extern __shared__ float4 spmv_lds[];
#ifdef MRGS_SPMV_TRACE
#define MRGS_SPMV_TRACE_PTR trace_ptr
#endif
__device__ __forceinline__ void csr_spmv3_sym_body(int block, const SpmvSeg& S, const uint64_t* __restrict__ sym, unsigned long long* trace_ptr)
{
    constexpr int NW = MRGS_SPMV_SYM_WAVES, D = MRGS_SPMV_SYM_DEPTH;
#ifdef MRGS_SPMV_TRACE
    const unsigned long long tr0 = wall_clock64();
#endif
    const int t = block / 12, ig = block - t * 12;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int L = S.log2n, N = 1 << L;
    const uint32_t p0 = S.panel_ptr[t], nq = S.panel_ptr[t + 1] - p0;                  // the tile's panel: 4 x 4 texel patches
    const uint2* __restrict__ A = reinterpret_cast<const uint2*>(S.val) + (size_t)p0 * 64;     // [patch][lane] -> four 16-bit weights, one per row of the patch
    const uint16_t* __restrict__ psrc = S.panel_src + p0;
    // staging role of the lane: texel kk of the patch's 16 (row kk >> 2, column kk & 3) under symmetry 4 ig + (lane >> 4).  The image of a
    // patch is a patch -- four runs of 48 bytes whichever way the symmetry turns the face (a run of 16 texels along x became 16 lines when
    // the axes were exchanged; the lines fetched into L1, 128 bytes for every 12 used, bounded the kernel: measured, round 5)
    const uint32_t kk = (uint32_t)lane & 15u, simg = (uint32_t)lane >> 4;
    const uint64_t tab = sym[4 * ig + (int)simg];
    float* Bs = reinterpret_cast<float*>(spmv_lds) + wave * (16 * MRGS_SPMV_SYM_BROW);     // (LDS serves a wave's accesses in order: no barrier between its write and its reads)
    const int LP = L - 2;                                               // patches per face edge = N / 4
    auto texel_of = [&](uint32_t cb) {
        const uint32_t x = 4u * (cb & (uint32_t)((1 << LP) - 1)) + (kk & 3u), y = 4u * ((cb >> LP) & (uint32_t)((1 << LP) - 1)) + (kk >> 2), s = cb >> (2 * LP);
        const uint32_t e = (uint32_t)(tab >> (6u * s)) & 63u;
        const uint32_t yy = (e & 16u) ? (uint32_t)(N - 1) - y : y, xx = (e & 32u) ? (uint32_t)(N - 1) - x : x;
        return ((((e & 7u) << L) + ((e & 8u) ? xx : yy)) << L) + ((e & 8u) ? yy : xx);
    };
    // software pipeline over the wave's steps: step i = patch wave + NW i of the panel, texels and weights of D steps in flight.  The loop
    // is unrolled D times over statically named stages: a stage's registers are the targets of loads in flight, and moving them down a
    // ring would wait for every one of them (it did: 0.35 us a step, per-wave timestamps, round 5).
    const uint32_t ni = nq > (uint32_t)wave ? (nq - (uint32_t)wave + (uint32_t)NW - 1u) / (uint32_t)NW : 0u;      // the wave's steps (<= 128)
    // the patch ids of all its steps in two VECTOR loads (lane j: steps j and 64 + j), read back per step with v_readlane -- as scalar loads
    // in the loop they would share the LDS reads' counter (lgkmcnt) and make every step wait for a scalar-cache miss
    const uint32_t q0 = (uint32_t)wave + (uint32_t)NW * (uint32_t)lane, q1 = q0 + 64u * (uint32_t)NW;
    const uint32_t ids0 = q0 < nq ? (uint32_t)psrc[q0] : 0u, ids1 = q1 < nq ? (uint32_t)psrc[q1] : 0u;
    auto patch_of = [&](uint32_t i) {      // (i uniform; beyond the wave's steps: patch 0, whose weights the step then zeroes)
        const uint32_t j = i < 127u ? i : 127u;
        return j < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)ids0, (int)j) : (uint32_t)__builtin_amdgcn_readlane((int)ids1, (int)(j - 64u));
    };
    struct Step { float f, v0, v1, v2; uint2 a4; };
    auto gather = [&](uint32_t i) {
        Step st;
        const uint32_t tex = texel_of(patch_of(i));
        st.f = S.pre[tex];
        const float* __restrict__ src = S.x + 3u * tex;
        st.v0 = src[0]; st.v1 = src[1]; st.v2 = src[2];
        const uint32_t qd = (uint32_t)wave + (uint32_t)NW * i;
        st.a4 = A[(size_t)(qd < nq ? qd : nq - 1u) * 64 + lane];
        return st;
    };
    // (the epilogue's row and its factor are asked for now: two dependent loads off the end of the workgroup's life)
    const uint32_t r_first = S.tile_ptr[t], r_end = S.tile_ptr[t + 1];
    const int orow_t = (int)threadIdx.x >> 4, ocol = threadIdx.x & 15;
    int orow = -1;
    if (threadIdx.x < 256 && (ocol & 3) < 3 && r_first + (uint32_t)orow_t < r_end) orow = S.image_rows[(r_first + (uint32_t)orow_t) * 48 + 4 * ig + (ocol >> 2)];
    const float opost = orow >= 0 ? S.row_scale[orow] : 0.0f;
    Step st[D];
#pragma unroll
    for (int j = 0; j < D; ++j) st[j] = gather((uint32_t)j);
    spmv_f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = spmv_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#ifdef MRGS_SPMV_TRACE
    unsigned long long tr1 = 0, tr2 = 0;
    { float probe = st[0].f + st[0].v0 + (float)st[0].a4.x; asm volatile("" :: "v"(probe)); tr1 = wall_clock64(); }
#endif
    float4* Bw = reinterpret_cast<float4*>(Bs + kk * MRGS_SPMV_SYM_BROW) + simg;        // [texel kk][symmetry][4] = [kk][16 columns], rows padded
    const float* Br = Bs + (lane >> 4) * MRGS_SPMV_SYM_BROW + (lane & 15);               // B[k = lane >> 4][column lane & 15] of a patch row
    for (uint32_t i0 = 0; i0 < ni; i0 += (uint32_t)D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            // this step: the wave's 16 texels x 4 symmetries into its buffer, four MFMAs out of it (a step past the wave's last has zero weights)
            const Step c0 = st[u];
            const bool live = i0 + (uint32_t)u < ni;
            const uint32_t ax = live ? c0.a4.x : 0u, ay = live ? c0.a4.y : 0u;
            *Bw = make_float4(c0.f * c0.v0, c0.f * c0.v1, c0.f * c0.v2, 0.0f);
            const float b0 = Br[0], b1 = Br[4 * MRGS_SPMV_SYM_BROW], b2 = Br[8 * MRGS_SPMV_SYM_BROW], b3 = Br[12 * MRGS_SPMV_SYM_BROW];
            st[u] = gather(i0 + (uint32_t)(u + D));
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)(ax & 0xFFFFu), b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)(ax >> 16), b1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)(ay & 0xFFFFu), b2, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)(ay >> 16), b3, acc[3], 0, 0, 0);
        }
    }
#ifdef MRGS_SPMV_TRACE
    { float probe = acc[0][0] + acc[1][0] + acc[2][0] + acc[3][0]; asm volatile("" :: "v"(probe)); tr2 = wall_clock64(); }
#endif
    // the waves' partial tiles -> one; C/D of the MFMA: column lane & 15, rows 4 (lane >> 4) + register
    float* red = reinterpret_cast<float*>(spmv_lds) + NW * (16 * MRGS_SPMV_SYM_BROW);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        red[wave * 256 + (4 * (lane >> 4) + r) * 16 + (lane & 15)] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    __syncthreads();
    if (orow >= 0) {      // (-1: a texel on the triangle's diagonal is its own image under one reflection -- written once)
        float sum = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += red[w * 256 + orow_t * 16 + ocol];
        S.y[3 * (size_t)orow + (ocol & 3)] = sum * opost;
    }
#ifdef MRGS_SPMV_TRACE
    if (MRGS_SPMV_TRACE_PTR != nullptr && lane == 0) {
        unsigned long long* o = MRGS_SPMV_TRACE_PTR + ((size_t)blockIdx.x * NW + wave) * 4;
        o[0] = tr0; o[1] = tr1; o[2] = tr2; o[3] = wall_clock64();
    }
#endif
}

__global__ void __launch_bounds__(MRGS_SPMV_BATCH_THREADS) csr_spmv3_batched_kernel(SpmvBatch B)
{
    int i = 0;
    for (int k = 1; k < B.n; ++k) i = ((int)blockIdx.x >= B.seg[k].first_block) ? k : i;
    const SpmvSeg& S = B.seg[i];
    const int own = (int)blockIdx.x - S.first_block;
    // (the row-per-wave bodies count 256-thread blocks: block 2 own + (threadIdx.x >> 8), which is what their `block * 256 + threadIdx.x` makes of 2 own)
    const int blk = S.fmt == 16 ? own : own * (MRGS_SPMV_BATCH_THREADS / 256);
    switch (S.fmt) {   // bit 2: 64 lanes per row (else 4); bit 1: 32-bit column indices (else 16); bit 0: fp32 weights (else 16-bit fixed point); 8: blocked rows; 16: blocked rows of one fundamental domain
    case 16: csr_spmv3_sym_body(blk, S, B.sym, B.trace); break;
    case 8: csr_spmv3_blk4_body(blk, S.nrows, S.row_ptr, (const uint16_t*)S.col, (const uint2*)S.val, S.row_scale, S.x, S.y); break;
    case 0: csr_spmv3_body<4, uint16_t, uint16_t>(blk, S.nrows, S.row_ptr, (const uint16_t*)S.col, (const uint16_t*)S.val, S.row_scale, S.x, S.y); break;
    case 1: csr_spmv3_body<4, uint16_t, float>(blk, S.nrows, S.row_ptr, (const uint16_t*)S.col, (const float*)S.val, S.row_scale, S.x, S.y); break;
    case 2: csr_spmv3_body<4, uint32_t, uint16_t>(blk, S.nrows, S.row_ptr, (const uint32_t*)S.col, (const uint16_t*)S.val, S.row_scale, S.x, S.y); break;
    case 3: csr_spmv3_body<4, uint32_t, float>(blk, S.nrows, S.row_ptr, (const uint32_t*)S.col, (const float*)S.val, S.row_scale, S.x, S.y); break;
    case 4: csr_spmv3_body<64, uint16_t, uint16_t>(blk, S.nrows, S.row_ptr, (const uint16_t*)S.col, (const uint16_t*)S.val, S.row_scale, S.x, S.y); break;
    case 5: csr_spmv3_body<64, uint16_t, float>(blk, S.nrows, S.row_ptr, (const uint16_t*)S.col, (const float*)S.val, S.row_scale, S.x, S.y); break;
    case 6: csr_spmv3_body<64, uint32_t, uint16_t>(blk, S.nrows, S.row_ptr, (const uint32_t*)S.col, (const uint16_t*)S.val, S.row_scale, S.x, S.y); break;
    default: csr_spmv3_body<64, uint32_t, float>(blk, S.nrows, S.row_ptr, (const uint32_t*)S.col, (const float*)S.val, S.row_scale, S.x, S.y); break;
    }
}

// entry points of the products
extern "C" {

// The storage rule of one CSR product (mrgs_csr_spmv3, and a segment of mrgs_csr_spmv3_batched that is not a fundamental domain): index and
// weight widths, a row scale for fixed-point weights, and for blocked rows (val_bytes == 8: 16-bit block indices, 4 x 16-bit weights per
// block, x read in 16-byte pieces) 64 lanes per row, rows in fours and the alignment of x and val.  The pointers are non-null already.
static bool spmv_storage_ok(int nrows, int col_bytes, const void* val, int val_bytes, const float* row_scale, const float* x, int lanes_per_row)
{
    if ((col_bytes != 2 && col_bytes != 4) || (val_bytes != 2 && val_bytes != 4 && val_bytes != 8)) return false;
    if (val_bytes != 4 && !row_scale) return false;
    if (val_bytes == 8 && (col_bytes != 2 || lanes_per_row < 64 || (nrows & 3) || ((uintptr_t)x & 15u) || ((uintptr_t)val & 7u))) return false;
    return true;
}

int mrgs_csr_spmv3(int32_t nrows, const uint32_t* row_ptr, const void* col, int32_t col_bytes, const void* val, int32_t val_bytes,
                   const float* row_scale, const float* x, float* y, int32_t lanes_per_row, void* stream)
{
    if (nrows < 1 || !row_ptr || !col || !val || !x || !y) return MRGS_E_BAD_ARG;
    if (!spmv_storage_ok(nrows, col_bytes, val, val_bytes, row_scale, x, lanes_per_row)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (val_bytes == 8) {
        hipLaunchKernelGGL(csr_spmv3_blk4_kernel, dim3((unsigned)(((size_t)nrows * 64 + 255) / 256)), dim3(256), 0, st, nrows, row_ptr, (const uint16_t*)col,
                           (const uint2*)val, row_scale, x, y);
        return MRGS_LAUNCH_STATUS();
    }
    const bool wide = lanes_per_row >= 64;
    const dim3 g(wide ? (unsigned)(((size_t)nrows * 64 + 255) / 256) : (unsigned)(((size_t)nrows * 4 + 255) / 256)), b(256);
#define SPMV(G_, IDX_, WT_) hipLaunchKernelGGL((csr_spmv3_kernel<G_, IDX_, WT_>), g, b, 0, st, nrows, row_ptr, (const IDX_*)col, (const WT_*)val, row_scale, x, y)
    if (wide) {
        if (col_bytes == 2) { if (val_bytes == 2) SPMV(64, uint16_t, uint16_t); else SPMV(64, uint16_t, float); }
        else { if (val_bytes == 2) SPMV(64, uint32_t, uint16_t); else SPMV(64, uint32_t, float); }
    } else {
        if (col_bytes == 2) { if (val_bytes == 2) SPMV(4, uint16_t, uint16_t); else SPMV(4, uint16_t, float); }
        else { if (val_bytes == 2) SPMV(4, uint32_t, uint16_t); else SPMV(4, uint32_t, float); }
    }
#undef SPMV
    return MRGS_LAUNCH_STATUS();
}

int mrgs_cube_symmetry_rows(int32_t res, int32_t* rows)
{
    if (res < 1 || res > 1024 || !rows) return MRGS_E_BAD_ARG;
    const int n = 6 * res * res;
    for (int g = 0; g < 48; ++g)
        for (int t = 0; t < n; ++t) {
            const CubeImage o = cube_symmetry_image(g, res, t / (res * res), (t / res) % res, t % res);
            rows[(size_t)g * n + t] = (o.s * res + o.y) * res + o.x;
        }
    return MRGS_OK;
}

int mrgs_csr_spmv3_batched(const MrgsSpmvDesc* descs, int32_t n, void* stream)
{
    if (!descs || n < 1 || n > MRGS_SPMV_MAX_BATCH) return MRGS_E_BAD_ARG;
    static SpmvBatch proto = [] { SpmvBatch b = {}; cube_symmetry_table(b.sym); return b; }();
    SpmvBatch B = proto;
    B.n = n;
    int blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < n; ++i) {
        const MrgsSpmvDesc& d = descs[i];
        const bool sym = d.image_rows != nullptr;
        if (d.nrows < 1 || !d.val || !d.x || !d.y) return MRGS_E_BAD_ARG;
        SpmvSeg& S = B.seg[i];
        S.nrows = d.nrows;
        S.first_block = blocks;
        S.log2n = 0;
        S.row_ptr = d.row_ptr; S.col = d.col; S.val = d.val; S.row_scale = d.row_scale; S.x = d.x; S.y = d.y;
        S.image_rows = nullptr; S.pre = nullptr; S.tile_ptr = nullptr; S.panel_ptr = nullptr; S.panel_src = nullptr;
        if (sym) {
            // tiles of rows of one fundamental domain: a power-of-two face of 4 .. 128 texels (16-bit block indices), nrows = 6 res^2 texels
            int L = 0;
            while ((1 << L) < d.res) ++L;
            // (a wave of the product keeps the patch ids of its 128 steps in two registers: panels of at most 128 x its workgroup's waves)
            if (d.res < 4 || d.res > 128 || (1 << L) != d.res || d.nrows != 6 * d.res * d.res || d.n_tiles < 1 || !d.pre_scale || !d.row_scale ||
                !d.tile_ptr || !d.panel_ptr || !d.panel_src || ((uintptr_t)d.val & 7u) || d.max_panel < 1 || d.max_panel > MRGS_SPMV_MAX_PANEL)
                return MRGS_E_BAD_ARG;
            S.fmt = 16;
            S.log2n = L; S.image_rows = d.image_rows; S.pre = d.pre_scale; S.tile_ptr = d.tile_ptr; S.panel_ptr = d.panel_ptr; S.panel_src = d.panel_src;
            blocks += d.n_tiles * 12;
            lds = MRGS_SPMV_SYM_LDS;
            continue;
        }
        if (!d.row_ptr || !d.col || !spmv_storage_ok(d.nrows, d.col_bytes, d.val, d.val_bytes, d.row_scale, d.x, d.lanes_per_row)) return MRGS_E_BAD_ARG;
        const bool blk4 = d.val_bytes == 8;
        const bool wide = d.lanes_per_row >= 64;
        S.fmt = blk4 ? 8 : ((wide ? 4 : 0) | (d.col_bytes == 4 ? 2 : 0) | (d.val_bytes == 4 ? 1 : 0));
        blocks += (int)(((size_t)d.nrows * (wide ? 64 : 4) + MRGS_SPMV_BATCH_THREADS - 1) / MRGS_SPMV_BATCH_THREADS);
    }
    B.total_blocks = blocks;
    B.trace = nullptr;
#ifdef MRGS_SPMV_TRACE
    if (const char* tp = getenv("MRGS_SPMV_TRACE_BUF")) B.trace = (unsigned long long*)strtoull(tp, nullptr, 16);     // developer build: per-wave timestamps
#endif
    hipLaunchKernelGGL(csr_spmv3_batched_kernel, dim3((unsigned)blocks), dim3(MRGS_SPMV_BATCH_THREADS), lds, (hipStream_t)stream, B);
    return MRGS_LAUNCH_STATUS();
}

}   // extern "C"

// ---- the mip chain ---------------------------------------------------------------------------------------------------------------------
// 2x2 box mip of a [6, N, N, 3] cubemap (cubemap_mip.forward, scene/light_utils.py:68-69)
__global__ void __launch_bounds__(256) cubemap_mip_fwd_kernel(int Nout, const float* __restrict__ in, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 6 * Nout * Nout * 3) return;
    const int c = i % 3, x = (i / 3) % Nout, y = (i / (3 * Nout)) % Nout, s = i / (3 * Nout * Nout);
    const int N = 2 * Nout;
    const float* p = in + ((size_t)(s * N + 2 * y) * N + 2 * x) * 3 + c;
    out[i] = 0.25f * (p[0] + p[3] + p[(size_t)N * 3] + p[(size_t)N * 3 + 3]);
}
// cubemap_mip.backward (scene/light_utils.py:71-80): NOT the transpose of the box filter -- the reference samples 0.25 * dout
// with a seamless bilinear cube fetch at the texel-centre directions of the finer level; reproduced as is, accumulating
// into g_fine (which already holds the finer level's own gradient).
__global__ void __launch_bounds__(256) cubemap_mip_bwd_kernel(int N, const float* __restrict__ dout /*[6,N/2,N/2,3]*/, float* __restrict__ g_fine)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 6 * N * N) return;
    const int x = t % N, y = (t / N) % N, s = t / (N * N);
    const float gx = -1.0f + 1.0f / (float)N + (float)x * ((2.0f - 2.0f / (float)N) / (float)(N - 1));   // torch.linspace(-1+1/N, 1-1/N, N)
    const float gy = -1.0f + 1.0f / (float)N + (float)y * ((2.0f - 2.0f / (float)N) / (float)(N - 1));
    const f3 v = cm_normalize(face_to_dir(s, gx, gy));
    const FaceUV fu = dir_to_face(v);
    const Taps tp = cube_taps(fu, N / 2);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float a = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (tp.w[q] != 0.f) a += tp.w[q] * dout[(size_t)tp.idx[q] * 3 + c];
        g_fine[(size_t)t * 3 + c] += 0.25f * a;
    }
}

// The whole box-mip chain below one level in ONE launch (cubemap_mip.forward applied `steps` <= 3 times, scene/light.py:74-76): a
// thread owns one channel of one texel of the coarsest level and averages its 2^steps x 2^steps block bottom-up, writing every level on the
// way -- the same 2x2 sums in the same order as the level-by-level kernel above, so the values are bit-identical to it.
template <int LVL>
__device__ __forceinline__ float mip_block(const float* __restrict__ in, int N0, int s, int y, int x, int c, float* const* outs)
{
    if constexpr (LVL == 0) {
        return in[((size_t)(s * N0 + y) * N0 + x) * 3 + c];
    } else {
        const float p00 = mip_block<LVL - 1>(in, N0, s, 2 * y, 2 * x, c, outs), p01 = mip_block<LVL - 1>(in, N0, s, 2 * y, 2 * x + 1, c, outs);
        const float p10 = mip_block<LVL - 1>(in, N0, s, 2 * y + 1, 2 * x, c, outs), p11 = mip_block<LVL - 1>(in, N0, s, 2 * y + 1, 2 * x + 1, c, outs);
        const float v = 0.25f * (p00 + p01 + p10 + p11);
        const int N = N0 >> LVL;
        outs[LVL - 1][((size_t)(s * N + y) * N + x) * 3 + c] = v;
        return v;
    }
}
struct MipOuts { float* o[3]; };
// Three levels with FOUR lanes per texel of the coarsest one (a DPP quad): each lane averages a 4x4 quarter of the texel's 8x8 block
// bottom-up (16 loads in flight instead of 64 behind each other), lane 0 of the quad folds the four level-2 values in the level-by-level
// kernel's order ((p00 + p01) + p10) + p11 -- bit-identical to it (10 -> 5 us for the 128..16 chain).
__global__ void __launch_bounds__(256) cubemap_mip_chain3_fwd_kernel(int N0, const float* __restrict__ in, MipOuts outs)
{
    const int Nc = N0 >> 3;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const bool live = t < 6 * Nc * Nc * 3 * 4;
    const int q = t & 3, i = live ? t >> 2 : 0;
    const int c = i % 3, x = (i / 3) % Nc, y = (i / (3 * Nc)) % Nc, s = i / (3 * Nc * Nc);
    float* const o[3] = {outs.o[0], outs.o[1], outs.o[2]};
    // my level-2 texel: (2 y + q / 2, 2 x + q % 2); its level-1 texels and their level-0 blocks below
    const int y2 = 2 * y + (q >> 1), x2 = 2 * x + (q & 1);
    const float v2 = live ? mip_block<2>(in, N0, s, y2, x2, c, o) : 0.0f;       // writes levels 1 and 2
    const float p01 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v2), 0x55, 0xf, 0xf, false));   // quad_perm [1,1,1,1]
    const float p10 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v2), 0xAA, 0xf, 0xf, false));   // [2,2,2,2]
    const float p11 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v2), 0xFF, 0xf, 0xf, false));   // [3,3,3,3]
    if (live && q == 0) o[2][((size_t)(s * Nc + y) * Nc + x) * 3 + c] = 0.25f * (v2 + p01 + p10 + p11);
}
__global__ void __launch_bounds__(256) cubemap_mip_chain_fwd_kernel(int N0, int steps, const float* __restrict__ in, MipOuts outs)
{
    const int Nc = N0 >> steps;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 6 * Nc * Nc * 3) return;
    const int c = i % 3, x = (i / 3) % Nc, y = (i / (3 * Nc)) % Nc, s = i / (3 * Nc * Nc);
    float* const o[3] = {outs.o[0], outs.o[1], outs.o[2]};
    if (steps == 1) mip_block<1>(in, N0, s, y, x, c, o);
    else if (steps == 2) mip_block<2>(in, N0, s, y, x, c, o);
    else mip_block<3>(in, N0, s, y, x, c, o);
}

// entry points of the mip chain
extern "C" {

int mrgs_cubemap_mip_chain_forward(int32_t res_in, int32_t n_steps, const float* in, float* const* outs, void* stream)
{
    if (res_in < 2 || n_steps < 1 || !in || !outs || (res_in >> n_steps) < 1 || ((res_in >> n_steps) << n_steps) != res_in) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const float* src = in;
    int res = res_in, done = 0;
    while (done < n_steps) {                                   // three levels per launch
        const int steps = n_steps - done < 3 ? n_steps - done : 3;
        MipOuts o = {{nullptr, nullptr, nullptr}};
        for (int k = 0; k < steps; ++k) {
            if (!outs[done + k]) return MRGS_E_BAD_ARG;
            o.o[k] = outs[done + k];
        }
        const int Nc = res >> steps, n = 6 * Nc * Nc * 3;
        if (steps == 3) hipLaunchKernelGGL(cubemap_mip_chain3_fwd_kernel, dim3((4 * n + 255) / 256), dim3(256), 0, st, res, src, o);
        else hipLaunchKernelGGL(cubemap_mip_chain_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, res, steps, src, o);
        src = outs[done + steps - 1];
        res = Nc;
        done += steps;
    }
    return MRGS_LAUNCH_STATUS();
}

int mrgs_cubemap_mip_chain_backward(int32_t res0, int32_t n_levels, float* const* g, void* stream)
{
    if (res0 < 2 || n_levels < 1 || n_levels > MRGS_MAX_MIPS || !g || (res0 >> (n_levels - 1)) < 1) return MRGS_E_BAD_ARG;
    for (int k = 0; k < n_levels; ++k) if (!g[k]) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    // One launch per level, coarse to fine (3 x 6.6 us for 128..16).  Measured and dropped: the levels up to 64 x 64 in ONE workgroup behind
    // barriers (152 us: 24 576 texels x the cross-face tap arithmetic on one CU); one launch in which every level-0 texel gathers down
    // the pyramid (84 us: 21 tap set-ups per texel, 12.8 k instructions); and, round 5, ONE launch whose levels wait for each other on
    // device counters (blocks of a level behind those of the coarser one in the grid, one lane spinning, release / acquire at agent
    // scope between the levels: correct, bit-identical, also from two streams at once -- and 91 us: an agent-scope release or acquire
    // writes back or invalidates the XCD's WHOLE L2, once per block, in the middle of a backward pass whose other kernels' data it holds).
    for (int k = n_levels - 2; k >= 0; --k) {
        const int N = res0 >> k, n = 6 * N * N;
        hipLaunchKernelGGL(cubemap_mip_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, N, g[k + 1], g[k]);
    }
    return MRGS_LAUNCH_STATUS();
}

int mrgs_cubemap_mip_forward(int32_t res_out, const float* in, float* out, void* stream)
{
    if (res_out < 1 || !in || !out) return MRGS_E_BAD_ARG;
    const int n = 6 * res_out * res_out * 3;
    hipLaunchKernelGGL(cubemap_mip_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res_out, in, out);
    return MRGS_LAUNCH_STATUS();
}

int mrgs_cubemap_mip_backward(int32_t res_fine, const float* dout, float* g_fine, void* stream)
{
    if (res_fine < 2 || (res_fine & 1) || !dout || !g_fine) return MRGS_E_BAD_ARG;
    const int n = 6 * res_fine * res_fine;
    hipLaunchKernelGGL(cubemap_mip_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res_fine, dout, g_fine);
    return MRGS_LAUNCH_STATUS();
}

}   // extern "C"
