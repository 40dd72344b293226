// GaussianModel's reset family and its normal-propagation step (scene/gaussian_model.py:532-722; contract in include/mrgs.h).
//
// The reference runs every reset as a chain of about a dozen elementwise torch kernels with boolean-index writes and then
// replace_tensor_to_optimizer, which allocates and zeroes both Adam moments.  Here one launch serves up to eight parameter groups: per
// group the new raw values and, where the optimizer has stepped, two zeroed moment tensors.
//   grid    (blocks of 256 rows, items).  A block first takes its rows' four keep conditions -- one thread a row, 9 B read per row: the
//           raw reflection strength, the raw roughness, the exclusive byte -- into a 256-byte table, then streams its slab of the item:
//           256 w consecutive floats, lane l of a pass at element 256 k + l, so every load and store is a coalesced dword whatever w is.
//   traffic per element 4 B read (8 B with caller's uniforms) and 4 B written (12 B with moments).  Nothing is reused.
//   index   the slab's first element is row0 * w in 64 bits; inside the slab 32 bits serve (w <= 2^20).
// Built without contraction: JITTER is the fp32 chain `v + ((u a) 2 - a)` operation by operation, the decisions compare the fp32 sigmoid
// with the fp32 threshold.  The constants L(a) = log(a / (1 - a)) are taken in double on the host and rounded once.  ENLARGE takes
// log(exp(v) a) in double and rounds once: the device's fp32 logf alone was seen two units in the last place off at |x| ~ 5.7, more than
// the whole chain is allowed (tests/model_statement.py: enlarge_tol); the rule touches two floats a row (kernel times: DESIGN.md).
#include <math.h>
#include "mrgs_internal.h"
#include "mrgs_philox.h"

namespace {

constexpr int ROWS = 256;                       // rows per workgroup = threads per workgroup
constexpr int MAX_WIDTH = 1 << 20;              // 256 w must stay below 2^31 for the slab's 32-bit index
constexpr int KEEP_ALL = MRGS_RESET_KEEP_EXCLUSIVE | MRGS_RESET_KEEP_REFL_ABOVE | MRGS_RESET_KEEP_REFL_BELOW | MRGS_RESET_KEEP_ROUGH_ABOVE;

struct DevItem {
    const float* src;
    float* dst;
    float* m;
    float* v;
    const float* noise;
    int width, rule, keep, index;
    float a, b, constant;                       // fp32 images of a and b; L(a) for the rules that take it
};

struct DevArgs {
    long long P;
    const float* refl;
    const float* rough;
    const unsigned char* exclusive;
    float refl_thr, rough_thr;
    unsigned long long seed;
    DevItem item[MRGS_RESET_MAX_ITEMS];
};

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(ROWS) void model_reset_kernel(const DevArgs a)
{
    __shared__ unsigned char cond[ROWS];
    const DevItem& it = a.item[blockIdx.y];
    const long long row0 = (long long)blockIdx.x * ROWS;
    const int nrows = (int)min((long long)ROWS, a.P - row0);
    {
        const int t = threadIdx.x;
        unsigned c = 0u;
        if (t < nrows && it.keep) {
            const long long row = row0 + t;
            if ((it.keep & MRGS_RESET_KEEP_EXCLUSIVE) && a.exclusive[row]) c |= MRGS_RESET_KEEP_EXCLUSIVE;
            if (it.keep & (MRGS_RESET_KEEP_REFL_ABOVE | MRGS_RESET_KEEP_REFL_BELOW)) {
                const float s = sigmoid_f32(a.refl[row]);
                if (s > a.refl_thr) c |= MRGS_RESET_KEEP_REFL_ABOVE;
                if (s < a.refl_thr) c |= MRGS_RESET_KEEP_REFL_BELOW;
            }
            if ((it.keep & MRGS_RESET_KEEP_ROUGH_ABOVE) && sigmoid_f32(a.rough[row]) > a.rough_thr) c |= MRGS_RESET_KEEP_ROUGH_ABOVE;
        }
        cond[t] = (unsigned char)(c & (unsigned)it.keep);
    }
    __syncthreads();
    const unsigned w = (unsigned)it.width;
    const unsigned n = (unsigned)nrows * w;
    const long long base = row0 * (long long)w;
    const float* __restrict__ src = it.src + base;
    const float* __restrict__ noise = it.noise ? it.noise + base : nullptr;
    float* __restrict__ dst = it.dst + base;
    float* __restrict__ m = it.m ? it.m + base : nullptr;
    float* __restrict__ v2 = it.v ? it.v + base : nullptr;
    const bool random = it.rule == MRGS_RESET_JITTER || it.rule == MRGS_RESET_JITTER_CONST;
    for (unsigned e = threadIdx.x; e < n; e += ROWS) {
        const unsigned r = e / w, col = e - r * w;
        const float v = src[e];
        float out = v;
        if (!cond[r]) {
            float u = 0.0f;
            if (random) {
                if (noise) u = noise[e];
                else {
                    const long long row = row0 + r;
                    unsigned x0, x1;
                    philox_pair((unsigned)a.seed, (unsigned)(a.seed >> 32), (unsigned)row, (unsigned)((unsigned long long)row >> 32), col,
                                (unsigned)it.index, x0, x1);
                    u = (float)(x0 >> 8) * 0x1p-24f;                                   // [0, 1), exact
                }
            }
            switch (it.rule) {
            case MRGS_RESET_CAP: out = sigmoid_f32(v) > it.a ? it.constant : v; break;
            case MRGS_RESET_FLOOR: out = sigmoid_f32(v) < it.a ? it.constant : v; break;
            case MRGS_RESET_LIFT: out = sigmoid_f32(v) > it.a ? v : it.constant; break;
            case MRGS_RESET_CONST: out = it.constant; break;
            case MRGS_RESET_FILL: out = it.a; break;
            case MRGS_RESET_JITTER: out = v + ((u * it.a) * 2.0f - it.a); break;
            case MRGS_RESET_JITTER_CONST: {
                const float c = fminf(fmaxf(it.a + (u - 0.5f) * it.b, 0.0f), 1.0f);
                out = logf(c / (1.0f - c));
                break;
            }
            default: out = (float)log(exp((double)v) * (double)it.a); break;            // MRGS_RESET_ENLARGE: in double, rounded once
            }
        }
        dst[e] = out;
        if (m) { m[e] = 0.0f; v2[e] = 0.0f; }
    }
}

bool takes_logit(int rule) { return rule == MRGS_RESET_CAP || rule == MRGS_RESET_FLOOR || rule == MRGS_RESET_LIFT || rule == MRGS_RESET_CONST; }

}  // namespace

extern "C" int mrgs_model_reset(const MrgsResetConfig* cfg, const MrgsResetItem* items, int32_t n_items, void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsResetConfig)) return MRGS_E_BAD_ARG;
    if (!items || n_items < 1 || n_items > MRGS_RESET_MAX_ITEMS || cfg->P < 0) return MRGS_E_BAD_ARG;
    DevArgs a;
    a.P = cfg->P; a.refl = cfg->refl_raw; a.rough = cfg->rough_raw; a.exclusive = cfg->exclusive;
    a.refl_thr = cfg->refl_thr; a.rough_thr = cfg->rough_thr; a.seed = cfg->seed;
    for (int i = 0; i < MRGS_RESET_MAX_ITEMS; ++i) {
        const MrgsResetItem& s = items[i < n_items ? i : 0];                           // unused slots repeat the first: no stray values
        if (i < n_items) {
            if (s.width < 1 || s.rule < 0 || s.rule > MRGS_RESET_ENLARGE || (s.keep & ~KEEP_ALL)) return MRGS_E_BAD_ARG;
            if ((s.exp_avg_dst == nullptr) != (s.exp_avg_sq_dst == nullptr)) return MRGS_E_BAD_ARG;
            if ((s.keep & MRGS_RESET_KEEP_EXCLUSIVE) && !cfg->exclusive) return MRGS_E_BAD_ARG;
            if ((s.keep & (MRGS_RESET_KEEP_REFL_ABOVE | MRGS_RESET_KEEP_REFL_BELOW)) && !cfg->refl_raw) return MRGS_E_BAD_ARG;
            if ((s.keep & MRGS_RESET_KEEP_ROUGH_ABOVE) && !cfg->rough_raw) return MRGS_E_BAD_ARG;
            if (cfg->P > 0 && (!s.src || !s.dst)) return MRGS_E_BAD_ARG;
            if (takes_logit(s.rule) && !(s.a > 0.0 && s.a < 1.0)) return MRGS_E_BAD_ARG;
            if (s.width > MAX_WIDTH) return MRGS_E_UNSUPPORTED;
        }
        DevItem& d = a.item[i];
        d.src = s.src; d.dst = s.dst; d.m = s.exp_avg_dst; d.v = s.exp_avg_sq_dst; d.noise = s.noise;
        d.width = s.width; d.rule = s.rule; d.keep = s.keep; d.index = i;
        d.a = (float)s.a; d.b = (float)s.b;
        d.constant = takes_logit(s.rule) ? (float)log(s.a / (1.0 - s.a)) : 0.0f;
    }
    if (cfg->P == 0) return MRGS_OK;
    const long long blocks = (cfg->P + ROWS - 1) / ROWS;
    if (blocks > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
    model_reset_kernel<<<dim3((unsigned)blocks, (unsigned)n_items), ROWS, 0, (hipStream_t)stream>>>(a);
    // the library's one status path, written out (the macro's users are enumerated by tests/test_status.py, one call per file; this file's
    // failure path is covered by tests/test_model_reset.py)
    return mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__);
}
