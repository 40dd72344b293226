// mrgs_surfel_walk.h -- the device side of the surfel tracer's wave-wide walk: the beam of a packet of rays and its tests against a node's
// child boxes and a leaf's surfels, the two gatherers (st_gather_wide: 64 rays, one walk; st_gather_group: a 4x4 or 2x2 packet with the
// exact tests spread over the wave), the rule by which rays form packets, the lane <-> packet mapping and the developer counters.
// The hierarchy itself is built by mrgs_surfel_hier.hip.
//
// A second tree over the same Morton order for waves whose 64 rays run close together (an 8x8 block of mirror rays off a smooth
// surface): 64 children per node, stored one child per LANE (six rows of 64 floats), three to four levels for 10^5..10^7 surfels.
// The wave walks it ONCE for all its rays: a node's 64 child boxes arrive with six coalesced loads, lane c tests child c against the
// BEAM of the wave's rays (interval arithmetic over the rays' origins and inverse directions: conservative for every ray), one
// ballot names the children to enter.  Ten dependent round trips per candidate (in a 4-ary tree) become three, and the 4 x 64
// ray-box tests of a packet walking such a tree become one test per lane.  At the bottom the surviving surfels are visited one by one: their
// record is broadcast from the lane that loaded it for the beam test (v_readlane, or ds_bpermute in a smaller packet), every lane evaluates
// the exact hit for its own ray and inserts into its own buffer.  No ordering of the walk: the far bound of a packet only closes
// when all its lanes have full buffers, which a measurement with 32-entry buffers showed to be rare.
#pragma once
#include "mrgs_surfel_blend.h"

namespace {

// Developer counters of a wave's walks (-DST_PROFILE; st_trace_tile then writes them into `state` in place of its usual contents):
// hierarchy nodes tested, candidates visited, lanes that hit, 100 MHz ticks in node fetch + beam test and in the candidate loops.
// Without the switch every member is empty and the gatherers compile as if the calls were not there.
struct StProf {
    int nodes, tests, lanes; unsigned t_fetch, t_cand;
#ifdef ST_PROFILE
    unsigned long long t0;                  // when the wave began its block of rays
    __device__ __forceinline__ void begin() { t0 = wall_clock64(); }
    __device__ __forceinline__ void node() { ++nodes; }
    __device__ __forceinline__ void test() { ++tests; }
    __device__ __forceinline__ void hits(bool ok) { lanes += __popcll(__ballot(ok)); }
    __device__ __forceinline__ unsigned long long now() const { return wall_clock64(); }
    __device__ __forceinline__ void fetched(unsigned long long since) { t_fetch += (unsigned)(wall_clock64() - since); }
    __device__ __forceinline__ void tested(unsigned long long since) { t_cand += (unsigned)(wall_clock64() - since); }
#else
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void node() {}
    __device__ __forceinline__ void test() {}
    __device__ __forceinline__ void hits(bool) {}
    __device__ __forceinline__ unsigned long long now() const { return 0ull; }
    __device__ __forceinline__ void fetched(unsigned long long) {}
    __device__ __forceinline__ void tested(unsigned long long) {}
#endif
};

// ---- lanes and packets --------------------------------------------------------------------------------------------------------
// A wave's 64 rays are an 8x8 block of an image (`tiled`: lane = 8 y + x) or 64 consecutive rays.  Its four QUADRANTS are the 4x4 corners
// of the block (or runs of 16 rays), a quadrant's four GROUPS its 2x2 corners (or runs of 4).  Packet numbers: 0 = the whole wave,
// 1 + q = quadrant q, 5 + 4 q + g = group g of quadrant q.
__device__ __forceinline__ int st_lane_quad(bool tiled, int lane) { return tiled ? ((lane >> 2) & 1) + 2 * (lane >> 5) : lane >> 4; }
__device__ __forceinline__ int st_lane_sub(bool tiled, int lane) { return tiled ? ((lane >> 1) & 1) + 2 * ((lane >> 4) & 1) : (lane >> 2) & 3; }
__device__ __forceinline__ bool st_lane_in_packet(bool tiled, int lane, int pk)       // pk >= 1
{
    const int quad = st_lane_quad(tiled, lane), sub = st_lane_sub(tiled, lane);
    return pk <= 4 ? quad == pk - 1 : (quad == ((pk - 5) >> 2) && sub == ((pk - 5) & 3));
}
// (the inverse, packet and ray -> lane, has its one user in st_gather_group and must equal st_lane_quad / st_lane_sub)

// The beam of a wave's rays in its own frame: m = mean direction, (e1, e2) across it, origin at the mean ray origin.  Ray i is the line
// (u, v)(s) = (u0_i + k1_i s, v0_i + k2_i s) over the depth s along m, so the beam's cross-section at depth s lies inside
// [min u0 + min(k1 s), max u0 + max(k1 s)] x (same in v): interval arithmetic again, but on slopes and offsets that are SMALL for rays
// that run together (in world axes the same bound multiplies O(1) numbers and lets almost every box through -- measured: 2.5x more
// candidates than a walk in which every lane tests its own ray, 20x on diverging mirror rays).
struct StBeam {
    float oc[3], m[3], e1[3], e2[3], am[3], a1[3], a2[3];       // frame and |components| (for the extent of a box along each frame axis)
    float u0min, u0max, v0min, v0max, k1min, k1max, k2min, k2max;
};

__device__ __forceinline__ StBeam st_make_beam(bool on, float ox, float oy, float oz, float dx, float dy, float dz, float& s0, float& dm)
{
    StBeam B;
    const float cnt = wave_dpp_sum(on ? 1.0f : 0.0f);
    const float il = on ? 1.0f / sqrtf(dx * dx + dy * dy + dz * dz) : 0.0f;
    float mx = wave_dpp_sum(dx * il), my = wave_dpp_sum(dy * il), mz = wave_dpp_sum(dz * il);
    const float ml = 1.0f / sqrtf(mx * mx + my * my + mz * mz);
    mx *= ml; my *= ml; mz *= ml;
    B.oc[0] = wave_dpp_sum(on ? ox : 0.0f) / cnt; B.oc[1] = wave_dpp_sum(on ? oy : 0.0f) / cnt; B.oc[2] = wave_dpp_sum(on ? oz : 0.0f) / cnt;
    // e1 = m x (the axis m is least aligned with), e2 = m x e1
    const float ax = fabsf(mx), ay = fabsf(my), az = fabsf(mz);
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (ax <= ay && ax <= az) qx = 1.f; else if (ay <= az) qy = 1.f; else qz = 1.f;
    float e1x = my * qz - mz * qy, e1y = mz * qx - mx * qz, e1z = mx * qy - my * qx;
    const float el = 1.0f / sqrtf(e1x * e1x + e1y * e1y + e1z * e1z);
    e1x *= el; e1y *= el; e1z *= el;
    const float e2x = my * e1z - mz * e1y, e2y = mz * e1x - mx * e1z, e2z = mx * e1y - my * e1x;
    B.m[0] = mx; B.m[1] = my; B.m[2] = mz; B.e1[0] = e1x; B.e1[1] = e1y; B.e1[2] = e1z; B.e2[0] = e2x; B.e2[1] = e2y; B.e2[2] = e2z;
#pragma unroll
    for (int k = 0; k < 3; ++k) { B.am[k] = fabsf(B.m[k]); B.a1[k] = fabsf(B.e1[k]); B.a2[k] = fabsf(B.e2[k]); }
    dm = dx * mx + dy * my + dz * mz;                                           // > 0 for every ray of a wave that runs together
    const float rx = ox - B.oc[0], ry = oy - B.oc[1], rz = oz - B.oc[2];
    s0 = rx * mx + ry * my + rz * mz;                                           // depth of the ray's origin
    const float tau = -s0 / dm;                                                 // ray parameter where it crosses the plane s = 0
    const float px = rx + tau * dx, py = ry + tau * dy, pz = rz + tau * dz;
    const float u0 = px * e1x + py * e1y + pz * e1z, v0 = px * e2x + py * e2y + pz * e2z;
    const float k1 = (dx * e1x + dy * e1y + dz * e1z) / dm, k2 = (dx * e2x + dy * e2y + dz * e2z) / dm;
    B.u0min = wave_dpp_min(on ? u0 : INFINITY); B.u0max = wave_dpp_max(on ? u0 : -INFINITY);
    B.v0min = wave_dpp_min(on ? v0 : INFINITY); B.v0max = wave_dpp_max(on ? v0 : -INFINITY);
    B.k1min = wave_dpp_min(on ? k1 : INFINITY); B.k1max = wave_dpp_max(on ? k1 : -INFINITY);
    B.k2min = wave_dpp_min(on ? k2 : INFINITY); B.k2max = wave_dpp_max(on ? k2 : -INFINITY);
    return B;
}

// May ANY ray of the beam touch the box lo..hi at a depth not in front of s_prev?  Conservative: a ray that meets the box has a point
// in it, whose depth lies in [sa, sb] and whose lateral coordinates lie within the box's extent about its centre.
__device__ __forceinline__ bool st_beam_box(const StBeam& B, const float lo[3], const float hi[3], float s_prev, float s_far, float& near_depth)
{
    float sc = 0.f, uc = 0.f, vc = 0.f, rs = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float c = 0.5f * (lo[k] + hi[k]) - B.oc[k], h = 0.5f * (hi[k] - lo[k]);
        sc += c * B.m[k]; uc += c * B.e1[k]; vc += c * B.e2[k];
        rs += h * B.am[k]; r1 += h * B.a1[k]; r2 += h * B.a2[k];
    }
    const float sa = sc - rs, sb = sc + rs;
    const float umax = B.u0max + fmaxf(fmaxf(B.k1min * sa, B.k1min * sb), fmaxf(B.k1max * sa, B.k1max * sb));
    const float umin = B.u0min + fminf(fminf(B.k1min * sa, B.k1min * sb), fminf(B.k1max * sa, B.k1max * sb));
    const float vmax = B.v0max + fmaxf(fmaxf(B.k2min * sa, B.k2min * sb), fmaxf(B.k2max * sa, B.k2max * sb));
    const float vmin = B.v0min + fminf(fminf(B.k2min * sa, B.k2min * sb), fminf(B.k2max * sa, B.k2max * sb));
    const float eps = 1e-4f * (fabsf(sc) + rs + fabsf(uc) + r1 + fabsf(vc) + r2 + fabsf(umax) + fabsf(umin) + fabsf(vmax) + fabsf(vmin)) + 1e-30f;
    near_depth = sa - eps;
    return uc - r1 <= umax + eps && uc + r1 >= umin - eps && vc - r2 <= vmax + eps && vc + r2 >= vmin - eps && sb + eps >= s_prev && sa - eps <= s_far;
}

// The same question for a surfel itself (level 0): centre = its mean, extent along a frame axis e = ext (|A.e| + |B.e|) with A = s_u r_u,
// B = s_v r_v (the support function of the square |u|, |v| <= ext), ext = min(3, radius at which alpha falls below 1/255).
__device__ __forceinline__ bool st_beam_surfel(const StBeam& B, const float4 g0, const float4 g1, const float4 g2, float opacity, float s_prev, float s_far)
{
    const float ax = g0.w, ay = g1.x, az = g1.y, bx = g1.z, by = g1.w, bz = g2.x;
    const float ia = 1.0f / (ax * ax + ay * ay + az * az), ib = 1.0f / (bx * bx + by * by + bz * bz);      // a = r_u / s_u -> s_u r_u = a / (a.a)
    const float vis = 255.0f * opacity;
    if (!(vis > 1.0f)) return false;                                               // alpha < 1/255 everywhere
    const float ext = fminf(ST_EXTENT, sqrtf(2.0f * logf(vis)) * 1.0001f);
    const float cx = g0.x - B.oc[0], cy = g0.y - B.oc[1], cz = g0.z - B.oc[2];
    const float sc = cx * B.m[0] + cy * B.m[1] + cz * B.m[2], uc = cx * B.e1[0] + cy * B.e1[1] + cz * B.e1[2], vc = cx * B.e2[0] + cy * B.e2[1] + cz * B.e2[2];
    const float rs = ext * (fabsf(ax * B.m[0] + ay * B.m[1] + az * B.m[2]) * ia + fabsf(bx * B.m[0] + by * B.m[1] + bz * B.m[2]) * ib);
    const float r1 = ext * (fabsf(ax * B.e1[0] + ay * B.e1[1] + az * B.e1[2]) * ia + fabsf(bx * B.e1[0] + by * B.e1[1] + bz * B.e1[2]) * ib);
    const float r2 = ext * (fabsf(ax * B.e2[0] + ay * B.e2[1] + az * B.e2[2]) * ia + fabsf(bx * B.e2[0] + by * B.e2[1] + bz * B.e2[2]) * ib);
    const float sa = sc - rs, sb = sc + rs;
    const float umax = B.u0max + fmaxf(fmaxf(B.k1min * sa, B.k1min * sb), fmaxf(B.k1max * sa, B.k1max * sb));
    const float umin = B.u0min + fminf(fminf(B.k1min * sa, B.k1min * sb), fminf(B.k1max * sa, B.k1max * sb));
    const float vmax = B.v0max + fmaxf(fmaxf(B.k2min * sa, B.k2min * sb), fmaxf(B.k2max * sa, B.k2max * sb));
    const float vmin = B.v0min + fminf(fminf(B.k2min * sa, B.k2min * sb), fminf(B.k2max * sa, B.k2max * sb));
    const float eps = 1e-4f * (fabsf(sc) + rs + fabsf(uc) + r1 + fabsf(vc) + r2 + fabsf(umax) + fabsf(umin) + fabsf(vmax) + fabsf(vmin)) + 1e-30f;
    return uc - r1 <= umax + eps && uc + r1 >= umin - eps && vc - r2 <= vmax + eps && vc + r2 >= vmin - eps && sb + eps >= s_prev && sa - eps <= s_far;
}

// The 16-entry columns of the [slot][thread] LDS buffers hold a ray's nearest hits ascending in (t, id).  Does (t, id) come in front of a
// full column's last entry?
__device__ __forceinline__ bool st_beats_last(uint32_t (*kb_id)[ST_THREADS], float (*kb_t)[ST_THREADS], int col, float t, uint32_t id)
{
    const float lt = kb_t[ST_K - 1][col];
    return t < lt || (t == lt && id < kb_id[ST_K - 1][col]);
}

// (Measured and dropped, round 3: touching the cache lines of the next remaining sibling with one LDS-DMA instruction whenever the walk
// descends into a child -- 12 lines of boxes or the 32 lines of a leaf group, no registers -- so that the visit after this one would find
// them cached: st_trace_kernel<0> 570 -> 590 us, st_trace_rest_kernel<0> 750 -> 789 us; the walk's visits are not waiting for misses that a
// one-visit lead removes, and the extra instruction costs six more spilled registers in kernels that are at their budget.)
__device__ __forceinline__ int st_gather_wide(const StWide& W, const float* __restrict__ boxes, const unsigned long long* __restrict__ vmask,
                                              const float4* __restrict__ leaf, uint32_t (*kb_id)[ST_THREADS], float (*kb_t)[ST_THREADS], int tid,
                                              float ox, float oy, float oz, float dx, float dy, float dz,
                                              float prev_t, uint32_t prev_id, bool first_pass, bool on, StProf& prof)
{
    int n = 0;
    if (__ballot(on) == 0) return 0;
    const int lane = tid & 63;
    float s0, dm;
    const StBeam B = st_make_beam(on, ox, oy, oz, dx, dy, dz, s0, dm);
    const float s_prev = wave_dpp_min(on ? s0 + prev_t * dm : INFINITY);      // nothing in front of every lane's last blended hit is needed
    // behind s_far no lane needs anything: every active lane's buffer is full and its last entry lies in front (depth = s0 + t dm)
    float s_far = INFINITY;
    unsigned long long mask[SW_MAX_LEVELS] = {0, 0, 0, 0};
    int node[SW_MAX_LEVELS] = {0, 0, 0, 0};
    float near1 = 0.f, near2 = 0.f, near3 = 0.f;                             // per lane: near depth of its child at levels 1..3
    float4 rec0 = make_float4(0, 0, 0, 0), rec1 = rec0, rec2 = rec0, rec3 = rec0;   // lane c: record of surfel c of the current group
    int l = W.n - 1;
    bool fresh = true;                                                       // node[l] has not been tested yet
    // The descent -- test a fresh node, leave an exhausted one, enter the nearest remaining child -- is WRITTEN OUT here and in
    // st_gather_group and must stay equal but for the profile ticks: as shared functions (on a walk-state struct: 92 bytes more scratch;
    // on these locals by reference: same registers, another instruction stream) the walking kernels did not come out as measured.
    for (;;) {
        if (fresh) {
            prof.node();
            const int nd = __builtin_amdgcn_readfirstlane(W.off[l] + node[l]);
            bool h;
            if (l == 0) {                                                     // the surfels themselves, one per lane
                const float4* g = leaf + ((size_t)node[0] * 64 + lane) * 4;
                rec0 = g[0]; rec1 = g[1]; rec2 = g[2]; rec3 = g[3];
                h = st_beam_surfel(B, rec0, rec1, rec2, rec3.x, s_prev, s_far);
            } else {
                const float* bx = boxes + (size_t)nd * 384 + lane;
                const float lo[3] = {bx[0], bx[64], bx[128]}, hi[3] = {bx[192], bx[256], bx[320]};
                float nd_depth;
                h = st_beam_box(B, lo, hi, s_prev, s_far, nd_depth);
                if (l == 1) near1 = nd_depth; else if (l == 2) near2 = nd_depth; else near3 = nd_depth;
            }
            mask[l] = __ballot(h) & vmask[nd];
            fresh = false;
        }
        if (mask[l] == 0) {
            if (l == W.n - 1) break;
            ++l;
            continue;
        }
        if (l > 0) {                                                          // nearest remaining child first
            const float mine = l == 1 ? near1 : l == 2 ? near2 : near3;
            const float key = ((mask[l] >> lane) & 1ull) ? mine : INFINITY;
            const float nearest = wave_dpp_min(key);
            if (nearest > s_far) { mask[l] = 0; continue; }                   // and everything else at this node lies behind it
            const int c = __builtin_ctzll(__ballot(key == nearest));
            mask[l] &= ~(1ull << c);
            node[l - 1] = node[l] * 64 + c;
            --l;
            fresh = true;
            continue;
        }
        // level 0: the surviving surfels of this group, one by one.  Lane c holds surfel c's record since the beam test: it is
        // broadcast from there (v_readlane, no memory round trip -- a record fetched per candidate cost ~1 us of latency each)
        unsigned long long m = mask[0];
        mask[0] = 0;
        while (m) {
            const int c = __builtin_ctzll(m);
            m &= m - 1;
            auto bc = [c](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), c)); };
            const float4 h0 = make_float4(bc(rec0.x), bc(rec0.y), bc(rec0.z), bc(rec0.w)), h1 = make_float4(bc(rec1.x), bc(rec1.y), bc(rec1.z), bc(rec1.w));
            const float4 h2 = make_float4(bc(rec2.x), bc(rec2.y), bc(rec2.z), bc(rec2.w));
            float4 h3;
            h3.x = bc(rec3.x); h3.y = bc(rec3.y);
            prof.test();
            if (on) {
                const uint32_t id = __float_as_uint(h3.y);
                const StHit h = st_hit(h0, h1, h2, h3.x, ox, oy, oz, dx, dy, dz);
                bool take = h.ok && (first_pass || h.t > prev_t || (h.t == prev_t && id > prev_id));
                prof.hits(h.ok);
                if (take && n == ST_K) take = st_beats_last(kb_id, kb_t, tid, h.t, id);
                if (take) {     // sorted insertion (a register-resident buffer with branch-free insertion was measured: 0.72 instead of
                                // 1.0 us per candidate for the wave, but 243 VGPRs = one wave per SIMD, slower overall).  Written out: must
                                // equal the loop of st_gather_group; as one function the walking kernels come out with another schedule
                    int pos = n < ST_K ? n++ : ST_K - 1;
                    while (pos > 0) {
                        const float pt = kb_t[pos - 1][tid];
                        const uint32_t pid = kb_id[pos - 1][tid];
                        if (pt < h.t || (pt == h.t && pid < id)) break;
                        kb_t[pos][tid] = pt; kb_id[pos][tid] = pid;
                        --pos;
                    }
                    kb_t[pos][tid] = h.t; kb_id[pos][tid] = id;
                }
            }
        }
        s_far = wave_dpp_max(on ? (n == ST_K ? s0 + kb_t[ST_K - 1][tid] * dm : INFINITY) : -INFINITY) * (1.0f + 1e-5f) + 1e-30f;
    }
    return n;
}

// The same walk for a packet SMALLER than the wave -- a 4x4 quadrant (R = 16 rays) or a 2x2 group (R = 4) --, with the exact tests at
// the bottom spread over all 64 lanes: lane l = g R + i tests the g-th surviving surfel of the leaf group against ray i of the packet, so
// one step evaluates 64 / R candidates (measured on the mirror rays of a rendered view, 95 % of whose waves are such packets: a candidate
// hits 6 of a packet's ~20 rays, i.e. in st_gather_wide's layout two lanes in three idled through every hit evaluation, and a candidate
// cost the wave 1.5 us).  The surfel's record crosses from the lane that loaded it by ds_bpermute, the ray's data from the lane that
// owns it (once per walk).  Hits go into the owning lane's LDS column as before; lanes that hit for the SAME ray take turns, ordered by
// their rank among them (per-ray ranks from one ballot), so a step costs as many insertion rounds as its busiest ray has hits.  The
// buffers end up holding the same 16 nearest (t, id) keys in the same order whatever the order of insertion: outputs and the record are
// those of the one-candidate-a-step walk bit for bit.  kb_n: entries in every column (the owners' `n` of st_gather_wide, shared here).
__device__ __forceinline__ int st_gather_group(const StWide& W, const float* __restrict__ boxes, const unsigned long long* __restrict__ vmask,
                                               const float4* __restrict__ leaf, uint32_t (*kb_id)[ST_THREADS], float (*kb_t)[ST_THREADS],
                                               uint32_t* kb_n, int tid, int pk, bool tiled, float ox, float oy, float oz, float dx, float dy, float dz,
                                               float prev_t, uint32_t prev_id, bool first_pass, bool on, StProf& prof)
{
    if (__ballot(on) == 0) return 0;
    const int lane = tid & 63, wbase = tid & ~63;
    float s0, dm;
    const StBeam B = st_make_beam(on, ox, oy, oz, dx, dy, dz, s0, dm);
    const float s_prev = wave_dpp_min(on ? s0 + prev_t * dm : INFINITY);
    float s_far = INFINITY;
    // the gather layout: lane = grp * R + i; `own` = the lane that owns ray i of packet pk (the inverse of st_lane_quad / st_lane_sub)
    const bool quad_pk = pk <= 4;
    const int shift = quad_pk ? 4 : 2, G = 64 >> shift;
    const int grp = lane >> shift, i = lane & ((1 << shift) - 1);
    int own;                              // (written out: as a helper the walking kernels come out with another schedule)
    if (quad_pk) {
        const int q = pk - 1;
        own = tiled ? 8 * (4 * (q >> 1) + (i >> 2)) + 4 * (q & 1) + (i & 3) : 16 * q + i;
    } else {
        const int q = (pk - 5) >> 2, g2 = (pk - 5) & 3;
        own = tiled ? 8 * (4 * (q >> 1) + 2 * (g2 >> 1) + (i >> 1)) + 4 * (q & 1) + 2 * (g2 & 1) + (i & 1) : 16 * q + 4 * g2 + i;
    }
    auto from = [](int src_lane, float v) { return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane << 2, __builtin_bit_cast(int, v))); };
    const float rox = from(own, ox), roy = from(own, oy), roz = from(own, oz), rdx = from(own, dx), rdy = from(own, dy), rdz = from(own, dz);
    const float rprev_t = from(own, prev_t);
    const uint32_t rprev_id = (uint32_t)__builtin_amdgcn_ds_bpermute(own << 2, (int)prev_id);
    const bool ron = __builtin_amdgcn_ds_bpermute(own << 2, (int)on) != 0;
    const int col = wbase + own;
    const unsigned long long sib = (quad_pk ? 0x0001000100010001ull : 0x1111111111111111ull) << i;      // the lanes that share my ray
    const unsigned long long below = (1ull << lane) - 1ull;
    kb_n[tid] = 0u;
    wave_lds_sync();
    unsigned long long mask[SW_MAX_LEVELS] = {0, 0, 0, 0};
    int node[SW_MAX_LEVELS] = {0, 0, 0, 0};
    float near1 = 0.f, near2 = 0.f, near3 = 0.f;
    float4 rec0 = make_float4(0, 0, 0, 0), rec1 = rec0, rec2 = rec0, rec3 = rec0;
    int l = W.n - 1;
    bool fresh = true;
    for (;;) {                                                                // (the descent of st_gather_wide, written out)
        if (fresh) {
            const unsigned long long tf0 = prof.now();
            prof.node();
            const int nd = __builtin_amdgcn_readfirstlane(W.off[l] + node[l]);
            bool h;
            if (l == 0) {
                const float4* g = leaf + ((size_t)node[0] * 64 + lane) * 4;
                rec0 = g[0]; rec1 = g[1]; rec2 = g[2]; rec3 = g[3];
                h = st_beam_surfel(B, rec0, rec1, rec2, rec3.x, s_prev, s_far);
            } else {
                const float* bx = boxes + (size_t)nd * 384 + lane;
                const float lo[3] = {bx[0], bx[64], bx[128]}, hi[3] = {bx[192], bx[256], bx[320]};
                float nd_depth;
                h = st_beam_box(B, lo, hi, s_prev, s_far, nd_depth);
                if (l == 1) near1 = nd_depth; else if (l == 2) near2 = nd_depth; else near3 = nd_depth;
            }
            mask[l] = __ballot(h) & vmask[nd];
            fresh = false;
            prof.fetched(tf0);
        }
        if (mask[l] == 0) {
            if (l == W.n - 1) break;
            ++l;
            continue;
        }
        if (l > 0) {                                                          // nearest remaining child first
            const float mine = l == 1 ? near1 : l == 2 ? near2 : near3;
            const float key = ((mask[l] >> lane) & 1ull) ? mine : INFINITY;
            const float nearest = wave_dpp_min(key);
            if (nearest > s_far) { mask[l] = 0; continue; }
            const int c = __builtin_ctzll(__ballot(key == nearest));
            mask[l] &= ~(1ull << c);
            node[l - 1] = node[l] * 64 + c;
            --l;
            fresh = true;
            continue;
        }
        unsigned long long m = mask[0];
        mask[0] = 0;
        const unsigned long long tc0 = prof.now();
        while (m) {
            // the next G survivors, one per lane group
            int c = 0;
            bool have = false;
            for (int k = 0; k < G && m; ++k) {
                const int ck = __builtin_ctzll(m);
                m &= m - 1;
                if (grp == k) { c = ck; have = true; }
                prof.test();
            }
            const float4 h0 = make_float4(from(c, rec0.x), from(c, rec0.y), from(c, rec0.z), from(c, rec0.w));
            const float4 h1 = make_float4(from(c, rec1.x), from(c, rec1.y), from(c, rec1.z), from(c, rec1.w));
            const float4 h2 = make_float4(from(c, rec2.x), from(c, rec2.y), from(c, rec2.z), from(c, rec2.w));
            const float opac = from(c, rec3.x);
            const uint32_t id = __float_as_uint(from(c, rec3.y));
            const StHit h = st_hit(h0, h1, h2, opac, rox, roy, roz, rdx, rdy, rdz);
            const bool take = have && ron && h.ok && (first_pass || h.t > rprev_t || (h.t == rprev_t && id > rprev_id));
            const unsigned long long takers = __ballot(take);
            prof.hits(have && ron && h.ok);
            if (takers == 0) continue;
            const int rank = __popcll(takers & sib & below);                 // takers of my ray in the lane groups before mine
            for (int k = 0;; ++k) {
                const bool now = take && rank == k;
                if (__ballot(now) == 0) break;                                // (ranks are dense per ray)
                if (now) {
                    uint32_t n = kb_n[col];
                    bool ins = true;
                    if (n == ST_K) ins = st_beats_last(kb_id, kb_t, col, h.t, id);
                    if (ins) {     // (written out: must equal the insertion of st_gather_wide)
                        int pos = n < ST_K ? (int)n++ : ST_K - 1;
                        while (pos > 0) {
                            const float pt = kb_t[pos - 1][col];
                            const uint32_t pid = kb_id[pos - 1][col];
                            if (pt < h.t || (pt == h.t && pid < id)) break;
                            kb_t[pos][col] = pt; kb_id[pos][col] = pid;
                            --pos;
                        }
                        kb_t[pos][col] = h.t; kb_id[pos][col] = id;
                        kb_n[col] = n;
                    }
                }
                wave_lds_sync();
            }
        }
        prof.tested(tc0);
        s_far = wave_dpp_max(on ? (kb_n[tid] == ST_K ? s0 + kb_t[ST_K - 1][tid] * dm : INFINITY) : -INFINITY) * (1.0f + 1e-5f) + 1e-30f;
    }
    return on ? (int)kb_n[tid] : 0;
}

// Rays "run together" when their directions stay within a cone of ~5.7 degrees about their mean (1 - cos <= 0.005 for a block or a quadrant, 0.001 = 2.6 degrees for a 2x2 group: wider beams of grazing rays sweep thousands of surfels; measured on mirror rays off a rendered view: 16 ms at 25 degrees, 9.5 at 11 before and 3.65 -> 1.9 at 11 -> 4.4 after the rays left over got waves of their own) and their origins within 2 % of the
// scene's extent of their centre.  `on` selects the rays asked about; the answer is wave-uniform.
__device__ __forceinline__ bool st_run_together(float extent, float cone, bool on, float ox, float oy, float oz, float dx, float dy, float dz)
{
    const float cnt = wave_dpp_sum(on ? 1.0f : 0.0f);
    if (cnt < 1.0f) return false;
    const float il = on ? 1.0f / sqrtf(dx * dx + dy * dy + dz * dz) : 0.0f;
    const float ux = dx * il, uy = dy * il, uz = dz * il;
    float mx = wave_dpp_sum(ux), my = wave_dpp_sum(uy), mz = wave_dpp_sum(uz);
    const float ml = sqrtf(mx * mx + my * my + mz * mz);
    if (!(ml > 0.5f * cnt)) return false;
    mx /= ml; my /= ml; mz /= ml;
    const float worst = wave_dpp_max(on ? 1.0f - (ux * mx + uy * my + uz * mz) : 0.0f);
    const float cx = wave_dpp_sum(on ? ox : 0.0f) / cnt, cy = wave_dpp_sum(on ? oy : 0.0f) / cnt, cz = wave_dpp_sum(on ? oz : 0.0f) / cnt;
    const float spread = wave_dpp_max(on ? fmaxf(fabsf(ox - cx), fmaxf(fabsf(oy - cy), fabsf(oz - cz))) : 0.0f);
    return worst <= cone && spread <= 0.02f * extent;
}

// Packet of every lane: 0 = the whole wave, 1..4 = its quadrant (4x4 rays of the 8x8 block, or 16 consecutive rays), 5..20 = its
// 2x2 group inside the quadrant, -1 = the ray walks alone.  The coarsest grouping whose rays run together wins; `present` gets one bit
// per packet in use.
template <class Args>     // the trace kernels' argument block: its packets, wide, ray_width and the three cones are read
__device__ __forceinline__ int st_assign_packets(const Args& A, const float* __restrict__ boxes, const unsigned long long* __restrict__ vmask, bool on,
                                                 int lane, float ox, float oy, float oz, float dx, float dy, float dz, uint32_t& present)
{
    present = 0;
    if (!A.packets || __ballot(on) == 0) return -1;
    const int root = A.wide.off[A.wide.n - 1];                                // lane c: child c of the root of the wide hierarchy
    float extent = 0.0f;
    if (A.wide.n > 1) {
        const bool there = (vmask[root] >> lane) & 1ull;
        const float* bx = boxes + (size_t)root * 384 + lane;
        for (int k = 0; k < 3; ++k)
            extent = fmaxf(extent, wave_dpp_max(there ? bx[(3 + k) * 64] : -INFINITY) - wave_dpp_min(there ? bx[k * 64] : INFINITY));
    } else {
        extent = INFINITY;                                                    // <= 64 surfels: no scale to compare origins with
    }
    if (st_run_together(extent, A.cone, on, ox, oy, oz, dx, dy, dz)) { present = 1u; return 0; }
    const bool tiled = A.ray_width > 0;
    const int quad = st_lane_quad(tiled, lane), sub = st_lane_sub(tiled, lane);
    int mine = -1;
    for (int q = 0; q < 4; ++q) {
        const bool in_q = on && quad == q;
        if (__ballot(in_q) == 0) continue;
        if (st_run_together(extent, A.cone_quad, in_q, ox, oy, oz, dx, dy, dz)) {
            if (in_q) mine = 1 + q;
            present |= 1u << (1 + q);
            continue;
        }
        for (int g = 0; g < 4; ++g) {
            const bool in_g = in_q && sub == g;
            if (__ballot(in_g) == 0) continue;
            if (st_run_together(extent, A.cone_group, in_g, ox, oy, oz, dx, dy, dz)) {
                if (in_g) mine = 5 + 4 * q + g;
                present |= 1u << (5 + 4 * q + g);
            }
        }
    }
    return mine;
}

}   // namespace
