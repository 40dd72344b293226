// mrgs_philox.h -- the counter generator of the split offsets (mrgs_densify.hip, mrgs_env_densify.hip; contract in include/mrgs.h).
// Philox4x32-10 (Salmon et al., SC'11): no state, no dependence on the grid.
#pragma once
#include "mrgs_internal.h"

__device__ __forceinline__ void philox_pair(unsigned key0, unsigned key1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned& x0, unsigned& x1)
{
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ key0, n2 = hi0 ^ c3 ^ key1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        key0 += W0; key1 += W1;
    }
    x0 = c0; x1 = c1;
}

// two standard normals for counter (row lo, row hi, k, c3): u_i = ((x_i >> 8) + 1) 2^-24 in (0, 1], Box-Muller
__device__ __forceinline__ void normal_pair(unsigned long long seed, long long row, int k, float& z0, float& z1, unsigned c3 = 0u)
{
    unsigned x0, x1;
    philox_pair((unsigned)seed, (unsigned)(seed >> 32), (unsigned)row, (unsigned)((unsigned long long)row >> 32), (unsigned)k, c3, x0, x1);
    const float u0 = (float)((x0 >> 8) + 1u) * 0x1p-24f, u1 = (float)((x1 >> 8) + 1u) * 0x1p-24f;      // (0, 1], exact
    const float r = sqrtf(-2.0f * logf(u0));
    float s, c;
    sincospif(2.0f * u1, &s, &c);
    z0 = r * c; z1 = r * s;
}
