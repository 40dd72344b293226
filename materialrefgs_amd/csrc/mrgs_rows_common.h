// mrgs_rows_common.h -- what the passes that move whole rows of a list of tensors state in the same words.  For all three (the compaction of
// mrgs_optim.hip, mrgs_densify.hip, mrgs_env_densify.hip): the chunking of a tensor list into the tables of their gather / emit launches.
// For the two densifiers: the emit pass's table with its host-side checks, and the device expressions both policies start from.  Each
// file is built with its own contraction setting (Makefile) and these functions inherit it, so nothing here may be rewritten for one file
// without checking the others.
// Not here: the head of the row decision (g, s0, s1, ms, o, clone, split, faint; classify_row and row_eval).  The two files load its inputs
// at different points and keep its results in different places, and every shared form of it changed the generated code of
// densify_classify_kernel or env_stage4_kernel (`make X.s` against the parent), so each file keeps its own.
#pragma once
#include "mrgs_internal.h"

// the tensors of one emit launch (grid y = tensor)
struct EmitTable {
    const float* src[MRGS_COMPACT_MAX_TENSORS];
    float* dst[MRGS_COMPACT_MAX_TENSORS];
    int row_floats[MRGS_COMPACT_MAX_TENSORS];
    int role[MRGS_COMPACT_MAX_TENSORS];
};

// The tensor list of an emit call, and the three raw pointers of its cfg that role XYZ reads.  empty: every destination is empty, so its
// pointer may be NULL.
static inline int densify_check_tensors(const MrgsDensifyTensor* tensors, int32_t n_tensors, bool empty, const float* xyz_raw,
                                        const float* scaling_raw, const float* rotation_raw)
{
    bool needs_xyz = false;
    for (int32_t i = 0; i < n_tensors; ++i) {
        const MrgsDensifyTensor& e = tensors[i];
        if (e.row_floats < 0 || e.row_floats > (1 << 20) || e.role < MRGS_DENSIFY_COPY || e.role > MRGS_DENSIFY_SCALING) return MRGS_E_BAD_ARG;
        if (e.row_floats == 0) continue;
        if (!e.src || (!e.dst && !empty)) return MRGS_E_BAD_ARG;
        if (e.role == MRGS_DENSIFY_XYZ) { if (e.row_floats != 3) return MRGS_E_BAD_ARG; needs_xyz = true; }
        if (e.role == MRGS_DENSIFY_SCALING) { if (e.row_floats != 2) return MRGS_E_BAD_ARG; }
    }
    if (needs_xyz && (!xyz_raw || !scaling_raw || !rotation_raw)) return MRGS_E_BAD_ARG;
    return MRGS_OK;
}

// launch(table, m) for every chunk of MRGS_COMPACT_MAX_TENSORS list entries that has m > 0 tensors with rows to move; false when there was none.
// fill(table, slot, entry) copies one list entry into the table.  The whole list is validated BEFORE this is called: a launch cannot be recalled.
template <typename Table, typename Tensor, typename Fill, typename Launch>
static inline bool tensor_table_chunks(const Tensor* tensors, int32_t n_tensors, Fill fill, Launch launch)
{
    bool any = false;
    for (int32_t first = 0; first < n_tensors; first += MRGS_COMPACT_MAX_TENSORS) {
        Table t;
        int m = 0;
        for (int32_t i = first; i < n_tensors && i < first + MRGS_COMPACT_MAX_TENSORS; ++i)
            if (tensors[i].row_floats != 0) fill(t, m++, tensors[i]);
        if (m == 0) continue;
        launch(t, m);
        any = true;
    }
    return any;
}
static inline void emit_table_fill(EmitTable& t, int m, const MrgsDensifyTensor& e)
{
    t.src[m] = e.src; t.dst[m] = e.dst; t.row_floats[m] = e.row_floats; t.role[m] = e.role;
}

// R[col][0] and R[col][1] of R(normalize(q)), q = (r, x, y, z): the two matrix entries a surfel's in-plane offset meets (build_rotation).
// By value: with reference outputs both emit kernels came out with another register allocation.
struct RotationRow2 { float R0, R1; };
__device__ __forceinline__ RotationRow2 rotation_row2(const float* q, int col)
{
    const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    float R0, R1;
    if (col == 0) { R0 = 1.0f - 2.0f * (y * y + z * z); R1 = 2.0f * (x * y - r * z); }
    else if (col == 1) { R0 = 2.0f * (x * y + r * z); R1 = 1.0f - 2.0f * (x * x + z * z); }
    else { R0 = 2.0f * (x * z - r * y); R1 = 2.0f * (y * z + r * x); }
    return {R0, R1};
}

// the statistics of visible row i that both models keep: accum += the 2-norm of all three gradient columns, denom += 1
__device__ __forceinline__ void densify_stats_row(const float* grad, long long i, float* accum, float* denom)
{
    const float gx = grad[3 * i], gy = grad[3 * i + 1], gz = grad[3 * i + 2];
    accum[i] += sqrtf(gx * gx + gy * gy + gz * gz);
    denom[i] += 1.0f;
}
