// mrgs_cc.h -- lock-free union-find over an int32 parent array in global memory: the connected components of the mesh's vertices
// (mrgs_mesh.hip) and of the edge mask's candidate pixels (mrgs_edges.hip).  A link always points to a smaller index, so the root of a
// component is its smallest member and the result is a set: it does not depend on the order in which the atomics land.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int cc_find(int* parent, int v)
{
    for (;;) {                                                          // links only ever point to a smaller index: the walk ends
        const int p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == v) return v;
        v = p;
    }
}
__device__ __forceinline__ void cc_union(int* parent, int x, int y)
{
    for (;;) {
        x = cc_find(parent, x); y = cc_find(parent, y);
        if (x == y) return;
        if (x < y) { const int s = x; x = y; y = s; }                   // hook the larger root under the smaller
        if (atomicCAS(parent + x, x, y) == x) return;                   // lost: x is no root any more, someone else made progress
    }
}
