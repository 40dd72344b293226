// The training contact sheet: save_training_vis (train_refreal.py:1513-1620, the same in train_refnerf.py and train_glossy.py) from the
// render's maps to the bytes of the PNG.
//
// What the reference runs per sheet -- abs / matmul / permute per derived image, four colour-map helpers that each cross to the host through
// numpy and cv2 (utils/image_utils.py:65-93), torch.stack of up to 23 fp32 images, torchvision's make_grid, F.interpolate to 2400 rows and
// save_image's mul / add / clamp / permute / to(uint8) -- is here
//   sheet_stats_kernel   per-workgroup minimum / maximum of every DEPTH and DEPTH2 cell, and for DEPTH2 the count, sum and sum of squares
//                        of (x - K) in double, K = the map's first value (only launched when there is such a cell)
//   sheet_rgb8_kernel    OUTPUT-DRIVEN: a workgroup owns up to 1024 pixels of one output row, maps each to its grid pixel (F.interpolate's
//                        legacy nearest), that to a border, an empty place or a pixel of a cell (make_grid's placement), evaluates the
//                        cell's rule there and stores the bytes through LDS as whole dwords
// There is no stack, no grid tensor and no resampled tensor, and nothing is read by the host.
//
// Arithmetic: fp32, every product and sum rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn: the file keeps the default flags, as
// mrgs_eval.hip whose byte rules it shares through mrgs_rgb8.h); DEPTH's and DEPTH2's division is the correctly rounded one.  DEPTH2's
// standard deviation is the population one, accumulated in double (shifted by K, so a constant map gives exactly 0), rounded once to fp32
// and multiplied by 6.f in fp32.  NaN gives byte 0 / level 0 everywhere and is skipped by the statistics; a DEPTH2 map with an infinite
// value has no standard deviation (NaN) and is level 0 throughout, as numpy's clip against a NaN bound is NaN.
#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_rgb8.h"

namespace {

constexpr int SMM = 64;           // workgroups (= partial rows) per statistics cell: one wave folds a cell, a lane per row
constexpr int EMPTY = 0xff;       // mode of a place of the last grid row that holds no cell

struct SheetStat {                // one partial row, 32 bytes
    float mn, mx;
    double n, s1, s2;             // count, sum (x - K), sum (x - K)^2 over the values that are not NaN (DEPTH2 only, else 0)
};

struct SheetArgs {
    int H, W, n_cells, xmaps;
    int off, pitch_y, pitch_x;    // make_grid: the first cell's corner, the distance between corners (n_cells = 1: 0, H, W)
    int Hg, Wg, Ho, Wo, chunks;   // chunks: workgroups per output row
    int n_stat;
    float sy, sx;
    float rot[9];
    const void* a[MRGS_SHEET_MAX_CELLS];
    const void* b[MRGS_SHEET_MAX_CELLS];
    uint8_t mode[MRGS_SHEET_MAX_CELLS], channels[MRGS_SHEET_MAX_CELLS], elem[MRGS_SHEET_MAX_CELLS], stat_slot[MRGS_SHEET_MAX_CELLS];
    uint8_t stat_cell[MRGS_SHEET_MAX_CELLS];       // stat_cell[slot] = index of the cell
};

// the shift of DEPTH2's sums: the map's first value when it is finite
__device__ __forceinline__ float stat_shift(const float* d) { const float k = d[0]; return fabsf(k) < INFINITY ? k : 0.f; }

// grid (SMM, n_stat)
__global__ __launch_bounds__(256) void sheet_stats_kernel(SheetArgs a, SheetStat* __restrict__ partials)
{
    __shared__ float red[4][2];
    __shared__ double redd[4][3];
    const int tid = threadIdx.x, slot = blockIdx.y, k = a.stat_cell[slot];
    const float* __restrict__ d = static_cast<const float*>(a.a[k]);
    const bool sums = a.mode[k] == MRGS_SHEET_DEPTH2;                  // uniform
    const size_t HW = (size_t)a.H * a.W;
    const double K = sums ? (double)stat_shift(d) : 0.0;
    float mn = INFINITY, mx = -INFINITY;
    double n = 0.0, s1 = 0.0, s2 = 0.0;
    const size_t stride = (size_t)SMM * 256;
    size_t i = (size_t)blockIdx.x * 256 + tid;
    for (; i + 3 * stride < HW; i += 4 * stride) {                      // four loads in flight: 64 workgroups a map are latency, not bytes
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = d[i + j * stride];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mn = fminf(mn, v[j]); mx = fmaxf(mx, v[j]);
            if (sums && v[j] == v[j]) { const double t = (double)v[j] - K; n += 1.0; s1 += t; s2 += t * t; }
        }
    }
    for (; i < HW; i += stride) {
        const float v = d[i];
        mn = fminf(mn, v); mx = fmaxf(mx, v);
        if (sums && v == v) { const double t = (double)v - K; n += 1.0; s1 += t; s2 += t * t; }
    }
    const float2 r = block_minmax(mn, mx, tid, red);
    if (sums) {
        n = wave_shfl_sum(n); s1 = wave_shfl_sum(s1); s2 = wave_shfl_sum(s2);
        if ((tid & 63) == 0) { redd[tid >> 6][0] = n; redd[tid >> 6][1] = s1; redd[tid >> 6][2] = s2; }
        __syncthreads();
    }
    if (tid == 0) {
        SheetStat p = {r.x, r.y, 0.0, 0.0, 0.0};
        if (sums) {                                                     // the order of the additions is fixed
            p.n = (redd[0][0] + redd[1][0]) + (redd[2][0] + redd[3][0]);
            p.s1 = (redd[0][1] + redd[1][1]) + (redd[2][1] + redd[3][1]);
            p.s2 = (redd[0][2] + redd[1][2]) + (redd[2][2] + redd[3][2]);
        }
        partials[(size_t)slot * SMM + blockIdx.x] = p;
    }
}

// min((int)floorf(dst * s), in - 1): the source index of F.interpolate's default nearest, one fp32 multiply (s > 0 is checked by the host)
__device__ __forceinline__ int nearest_src(int dst, float s, int in)
{
    const float f = floorf(__fmul_rn((float)dst, s));
    const int i = f < 2147483648.f ? (int)f : 0x7fffffff;
    return i < in - 1 ? i : in - 1;
}

// grid (Ho * chunks): workgroup b owns pixels [x0, x0 + n) of output row b / chunks, x0 = (b % chunks) * XCHUNK.  LDS holds the run's 3 n
// bytes shifted by the first byte's global offset & 3 (mrgs_rgb8.h: store_lds_bytes), and per grid column of cells what a pixel needs of
// its cell: the two planes, the mode, and for DEPTH / DEPTH2 the minimum, the denominator and the clip -- read (and, for the statistics,
// folded from the first launch's partial rows) once per workgroup by the wave the column falls to.
__global__ __launch_bounds__(256) void sheet_rgb8_kernel(SheetArgs a, const SheetStat* __restrict__ partials, uint8_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[3 * XCHUNK + 8];
    __shared__ const void* c_a[MRGS_SHEET_MAX_CELLS];
    __shared__ const void* c_b[MRGS_SHEET_MAX_CELLS];
    __shared__ uint32_t c_meta[MRGS_SHEET_MAX_CELLS];                   // mode | channels << 8 | elem << 16
    __shared__ float c_mn[MRGS_SHEET_MAX_CELLS], c_den[MRGS_SHEET_MAX_CELLS], c_hi[MRGS_SHEET_MAX_CELLS];
    const int tid = threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)a.chunks), x0 = (int)(blockIdx.x % (unsigned)a.chunks) * XCHUNK;
    const int n = a.Wo - x0 < XCHUNK ? a.Wo - x0 : XCHUNK;              // pixels of this run, >= 1
    const size_t obase = ((size_t)y * a.Wo + x0) * 3;
    const int shift = (int)(obase & 3);
    const size_t HW = (size_t)a.H * a.W;
    // the row of the grid and of the cells this output row shows (uniform)
    const int ty = nearest_src(y, a.sy, a.Hg) - a.off;
    const int cy = ty >= 0 ? ty / a.pitch_y : 0;
    const int ry = ty - cy * a.pitch_y;
    const bool row_live = (ty >= 0) & (ry < a.H);                       // else a border row: all zero
    if (row_live) {
        // the columns of cells the run touches: source indices grow with the output index
        const int t0 = nearest_src(x0, a.sx, a.Wg) - a.off, t1 = nearest_src(x0 + n - 1, a.sx, a.Wg) - a.off;
        const int cx0 = t0 > 0 ? t0 / a.pitch_x : 0;
        int cx1 = t1 > 0 ? t1 / a.pitch_x : 0;
        cx1 = cx1 < a.xmaps - 1 ? cx1 : a.xmaps - 1;
        const int lane = tid & 63;
        for (int cx = cx0 + (tid >> 6); cx <= cx1; cx += 4) {           // one wave per column
            const int k = cy * a.xmaps + cx;
            if (k >= a.n_cells) { if (lane == 0) c_meta[cx] = EMPTY; continue; }
            const int mode = a.mode[k];
            float mn = 0.f, den = 1.f, hi = INFINITY;
            if (mode == MRGS_SHEET_DEPTH || mode == MRGS_SHEET_DEPTH2) {
                const SheetStat p = partials[(size_t)a.stat_slot[k] * SMM + lane];
                mn = wave_shfl_min(p.mn);
                float mx = wave_shfl_max(p.mx);
                if (mode == MRGS_SHEET_DEPTH2) {
                    const double cnt = wave_shfl_sum(p.n), s1 = wave_shfl_sum(p.s1), s2 = wave_shfl_sum(p.s2);
                    double var = (s2 - s1 * s1 / cnt) / cnt;            // population variance, the shift cancels
                    var = var < 0.0 ? 0.0 : var;                        // (NaN stays NaN)
                    hi = __fmul_rn(6.f, (float)sqrt(var));              // 6 * std
                    // the clipped map's minimum and maximum are the clipped raw ones (the clip is monotone)
                    mn = hi == hi ? fminf(fmaxf(mn, 0.f), hi) : hi;
                    mx = hi == hi ? fminf(fmaxf(mx, 0.f), hi) : hi;
                }
                den = __fsub_rn(__fadd_rn(1e-20f, mx), mn);             // 1e-20 + depth.max() - depth.min()
            }
            if (lane == 0) {
                c_a[cx] = a.a[k]; c_b[cx] = a.b[k];
                c_meta[cx] = (uint32_t)mode | (uint32_t)a.channels[k] << 8 | (uint32_t)a.elem[k] << 16;
                c_mn[cx] = mn; c_den[cx] = den; c_hi[cx] = hi;
            }
        }
    }
    __syncthreads();
    const size_t rowoff = (size_t)ry * a.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j;
        if (i >= n) continue;
        uint32_t b0 = 0, b1 = 0, b2 = 0;
        const int tx = nearest_src(x0 + i, a.sx, a.Wg) - a.off;
        const int cx = tx >= 0 ? tx / a.pitch_x : 0;
        const int rx = tx - cx * a.pitch_x;
        if (row_live & (tx >= 0) & (rx < a.W)) {                        // cx < xmaps: Wg = pitch_x xmaps + off
            const uint32_t meta = c_meta[cx];
            const int mode = meta & 0xff;
            if (mode != EMPTY) {
                const size_t p = rowoff + rx;
                const float* __restrict__ fa = static_cast<const float*>(c_a[cx]);
                if (mode == MRGS_SHEET_UNIT) {
                    b0 = unit_byte(fa[p]);
                    if ((meta >> 8 & 0xff) == 3) { b1 = unit_byte(fa[HW + p]); b2 = unit_byte(fa[2 * HW + p]); }
                    else { b1 = b0; b2 = b0; }                          // .repeat(3, 1, 1)
                } else if (mode == MRGS_SHEET_ABSDIFF) {                // torch.abs(gt - render), :1518
                    const float* __restrict__ fb = static_cast<const float*>(c_b[cx]);
                    b0 = unit_byte(fabsf(__fsub_rn(fa[p], fb[p])));
                    b1 = unit_byte(fabsf(__fsub_rn(fa[HW + p], fb[HW + p])));
                    b2 = unit_byte(fabsf(__fsub_rn(fa[2 * HW + p], fb[2 * HW + p])));
                } else if (mode == MRGS_SHEET_NORMAL_VIEW) {            // (rot @ x)[[2, 1, 0]] * 0.5 + 0.5, :1521-1524
                    const float v0 = fa[p], v1 = fa[HW + p], v2 = fa[2 * HW + p];
                    float yv[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        yv[r] = __fadd_rn(__fadd_rn(__fmul_rn(a.rot[3 * r], v0), __fmul_rn(a.rot[3 * r + 1], v1)), __fmul_rn(a.rot[3 * r + 2], v2));
                    b0 = unit_byte(__fadd_rn(__fmul_rn(0.5f, yv[2]), 0.5f));
                    b1 = unit_byte(__fadd_rn(__fmul_rn(0.5f, yv[1]), 0.5f));
                    b2 = unit_byte(__fadd_rn(__fmul_rn(0.5f, yv[0]), 0.5f));
                } else {
                    uint32_t level;
                    if (mode == MRGS_SHEET_MASK) {                      // (d_mask.float() * 255).astype(uint8), image_utils.py:66
                        const float m = (meta >> 16 & 0xff) == MRGS_SHEET_ELEM_U8 ? (float)static_cast<const uint8_t*>(c_a[cx])[p] : fa[p];
                        level = to_byte(__fmul_rn(m, 255.f));
                    } else if (mode == MRGS_SHEET_LEVEL) {              // visualize_depth(norm=False)
                        level = to_byte(__fmul_rn(fa[p], 255.f));
                    } else {                                            // DEPTH, DEPTH2: image_utils.py:75-76, :86-89
                        float x = fa[p];
                        if (mode == MRGS_SHEET_DEPTH2) {
                            const float hi = c_hi[cx];
                            x = ((x == x) & (hi == hi)) ? fminf(fmaxf(x, 0.f), hi) : NAN;     // depth.clip(0, 6 * std)
                        }
                        level = to_byte(__fmul_rn(__fsub_rn(x, c_mn[cx]) / c_den[cx], 255.f));
                    }
                    b0 = d_jet.rgb[level][0]; b1 = d_jet.rgb[level][1]; b2 = d_jet.rgb[level][2];
                }
            }
        }
        sb[shift + 3 * i] = (uint8_t)b0; sb[shift + 3 * i + 1] = (uint8_t)b1; sb[shift + 3 * i + 2] = (uint8_t)b2;
    }
    __syncthreads();
    store_lds_bytes(sb, shift, 3 * n, out, obase, tid);
}

bool mode_is_stat(int mode) { return mode == MRGS_SHEET_DEPTH || mode == MRGS_SHEET_DEPTH2; }

}   // namespace

extern "C" size_t mrgs_sheet_ws_bytes(void) { return (size_t)MRGS_SHEET_MAX_CELLS * SMM * sizeof(SheetStat); }

extern "C" int mrgs_sheet_rgb8(const MrgsSheetConfig* cfg, const MrgsSheetCell* cells, void* ws, size_t ws_bytes, uint8_t* out, void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsSheetConfig) || cfg->flags != 0) return MRGS_E_BAD_ARG;
    if (cfg->H <= 0 || cfg->W <= 0 || cfg->Ho <= 0 || cfg->Wo <= 0 || cfg->nrow < 1 || cfg->padding < 0) return MRGS_E_BAD_ARG;
    if (cfg->n_cells < 1 || cfg->n_cells > MRGS_SHEET_MAX_CELLS || !cells || !out || (reinterpret_cast<uintptr_t>(out) & 3)) return MRGS_E_BAD_ARG;
    if (!(cfg->scale_y > 0.f) || !(cfg->scale_x > 0.f) || !(cfg->scale_y < INFINITY) || !(cfg->scale_x < INFINITY)) return MRGS_E_BAD_ARG;
    SheetArgs a = {};
    a.H = cfg->H; a.W = cfg->W; a.n_cells = cfg->n_cells; a.Ho = cfg->Ho; a.Wo = cfg->Wo;
    a.sy = cfg->scale_y; a.sx = cfg->scale_x;
    for (int i = 0; i < 9; ++i) a.rot[i] = cfg->rot[i];
    // torchvision.utils.make_grid: one image is returned as it is
    const int pad = a.n_cells > 1 ? cfg->padding : 0;
    a.xmaps = cfg->nrow < a.n_cells ? cfg->nrow : a.n_cells;
    const int ymaps = (a.n_cells + a.xmaps - 1) / a.xmaps;
    const int64_t pitch_y = (int64_t)a.H + pad, pitch_x = (int64_t)a.W + pad;
    const int64_t Hg = pitch_y * ymaps + pad, Wg = pitch_x * a.xmaps + pad;
    if (Hg > 0x7fffffff || Wg > 0x7fffffff || (int64_t)a.Ho * a.Wo * 3 > 0x7fffffff) return MRGS_E_BAD_ARG;
    a.off = pad; a.pitch_y = (int)pitch_y; a.pitch_x = (int)pitch_x; a.Hg = (int)Hg; a.Wg = (int)Wg;
    for (int k = 0; k < a.n_cells; ++k) {
        const MrgsSheetCell& c = cells[k];
        if (c.mode < MRGS_SHEET_UNIT || c.mode > MRGS_SHEET_MASK || !c.data) return MRGS_E_BAD_ARG;
        if (c.elem != MRGS_SHEET_ELEM_F32 && !(c.mode == MRGS_SHEET_MASK && c.elem == MRGS_SHEET_ELEM_U8)) return MRGS_E_BAD_ARG;
        if (c.elem == MRGS_SHEET_ELEM_F32 && (reinterpret_cast<uintptr_t>(c.data) & 3)) return MRGS_E_BAD_ARG;
        const bool three = c.mode == MRGS_SHEET_ABSDIFF || c.mode == MRGS_SHEET_NORMAL_VIEW;
        if (c.mode == MRGS_SHEET_UNIT ? (c.channels != 1 && c.channels != 3) : c.channels != (three ? 3 : 1)) return MRGS_E_BAD_ARG;
        if (c.mode == MRGS_SHEET_ABSDIFF && (!c.data2 || (reinterpret_cast<uintptr_t>(c.data2) & 3))) return MRGS_E_BAD_ARG;
        a.a[k] = c.data; a.b[k] = c.mode == MRGS_SHEET_ABSDIFF ? c.data2 : nullptr;
        a.mode[k] = (uint8_t)c.mode; a.channels[k] = (uint8_t)c.channels; a.elem[k] = (uint8_t)c.elem;
        if (mode_is_stat(c.mode)) { a.stat_slot[k] = (uint8_t)a.n_stat; a.stat_cell[a.n_stat++] = (uint8_t)k; }
    }
    if (a.n_stat && (!ws || (reinterpret_cast<uintptr_t>(ws) & 15))) return MRGS_E_BAD_ARG;
    if (a.n_stat && ws_bytes < mrgs_sheet_ws_bytes()) return MRGS_E_WORKSPACE;
    a.chunks = (a.Wo + XCHUNK - 1) / XCHUNK;
    if ((int64_t)a.chunks * a.Ho > 0x7fffffff) return MRGS_E_BAD_ARG;  // (implied by Ho Wo 3 <= int32; kept for the grid's sake)
    hipStream_t st = (hipStream_t)stream;
    if (a.n_stat) sheet_stats_kernel<<<dim3(SMM, a.n_stat), 256, 0, st>>>(a, (SheetStat*)ws);
    sheet_rgb8_kernel<<<dim3((unsigned)(a.chunks * a.Ho)), 256, 0, st>>>(a, (const SheetStat*)ws, out);
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}
