// Ray tracing of 2D-gaussian surfels (second half): the replacement of the un-vendored OptiX extension
// `diff_surfel_tracing` behind HardwareRendering (gaussian_renderer/optix_utils.py:14-271), whose callers trace the mirror rays of
// every pixel through the surfel set (render_indirect / render_surfel_with_envgs / render_surfel2, envgs_renderer.py:461-804).
//
// What the reference fixes and what it leaves open.  optix_utils.py fixes the primitive -- each surfel is the quad
// mean +- 3 s_u r_u +- 3 s_v r_v as two triangles (get_disks :36-66), rebuilt every training iteration (:68-82) --, the ray
// convention (direction NOT normalised, depth = ray parameter, :121-123), the inputs (means, opacities, scales / rotations, shs or
// colours, two "others" channels :173-183) and the outputs rgb, dpt, acc, norm, dist, aux, mid, wet (:185-197, 218-233).  The
// arithmetic between them lives in the missing extension: PARITY IS UNPINNED for this file.  It is defined here as the 2DGS
// compositing of the vendored rasterizer applied along a ray (forward.cu:366-420 with the ray parameter in place of the view depth):
//   hit of surfel p:  t = n.(m - o) / n.d,  x = o + t d,  u = r_u.(x - m) / s_u,  v = r_v.(x - m) / s_v,  t > 0, |u|,|v| <= 3
//   G = exp(-(u^2 + v^2) / 2),  alpha = min(0.99, opacity G),  skipped when alpha < 1/255
//   hits in order of (t, index);  w = alpha T;  the hit that would take T below 1e-4 is not blended and ends the ray
//   rgb = sum w c + T bg, dpt = sum w t, acc = sum w, norm = sum w n (turned against the ray), aux = sum w others,
//   dist = sum_i w_i (t_i^2 A_i + M2_i - 2 t_i M1_i)  (A, M1, M2: sums of w, w t, w t^2 over the hits before i), wet[p] += w.
// oracle/surfel_trace_oracle.py states the same definition densely (every ray against every surfel) in torch; its autograd is the
// check of the hand-written backward below.
//
// MI355X design.  No RT cores; what the machine has is 64 lanes per wave, scalar registers for what a wave shares, and LDS.
//  * THE HIERARCHY, a complete 64-ary tree over the Morton order, is built on the device every iteration: mrgs_surfel_hier.hip.
//    The walk over it is in mrgs_surfel_walk.h, the compositing arithmetic both directions share in mrgs_surfel_blend.h; this file
//    schedules them (two launches, lists, tickets, records) and holds the entry points.
//  * 64 RAYS, ONE WALK (st_gather_wide): a wave takes an 8x8 block of rays.  While they run together (directions within ~11 degrees,
//    origins close) the wave walks the tree once for all of them: lane c tests child c against the BEAM of the rays (bounds on offset
//    and slope in the rays' own frame), a ballot names the children to enter, the nearest first (wave-min of the near depths).  At the
//    bottom lane c tests surfel c's own square against the beam; the surviving surfels are visited one by one, their record broadcast
//    from lane c (v_readlane), every lane evaluating the exact hit for ITS ray and inserting into its own sorted 16-entry buffer
//    (LDS, [slot][lane]).  Blocks that do not run together split into 4x4 quadrants, then 2x2 groups; such a packet spreads the
//    exact tests over all 64 lanes, 64 / R candidates a step (st_gather_group).  The wave-wide minima / maxima / sums of the walk
//    (nearest child, far bound, beam) are DPP butterflies, not __shfl_xor (= ds_bpermute) ones.
//  * ONE RAY, ONE WAVE (st_trace_lone_rays): what is left over walks with the lanes turned sideways -- 64 children, then the 64
//    surfels of a leaf group, against the one ray -- instead of alone in a lane (a dependent ~1 us gather per step).
//  * 16-NEAREST PASSES: a ray gathers its 16 nearest not-yet-blended hits, blends them front to back, and continues behind the last
//    one while the buffer came back full and the ray is not saturated; the walk's far bound closes when every ray of the packet has
//    a full buffer.
//  * BACKWARD FRONT TO BACK as well: with the forward's totals at hand, d/d alpha_i = T_i q_i - (Q - Q_i) / (1 - alpha_i)
//    (q: the pixel gradient contracted with hit i's contribution, Q its weighted sum over all hits, Q_i over hits <= i), so the
//    backward re-walks exactly the forward's passes and needs no per-ray hit storage.
// What was measured on the way (800x800 primary rays through the 300 k shell scene, forward): a 4-ary tree walked per lane with the
// stack in registers 42 ms; + leaf-ordered records, 8x8 ray blocks 29; the same tree walked per wave (scalar node loads, every lane
// tests its ray) 10; 64-wide nodes with the beam test 4.8.  Mirror rays off a rendered view: 16 ms with a 25-degree cone, 9.5 with
// 11 degrees, 3.9 with the left-over rays traced one per wave.
// Compiled with -ffp-contract=off: forward and backward evaluate the hit expression identically.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_surfel_trace.h"
#include "mrgs_surfel_blend.h"
#include "mrgs_surfel_walk.h"

namespace {

struct StArgs {
    int64_t n_rays;
    const float* ray_o; const float* ray_d;
    const float4* geom;                   // [P][4]: (m.xyz, a.x) (a.yz, b.xy) (b.z, n.xyz) (opacity, -, -, -);  a = r_u / s_u, b = r_v / s_v
    const float4* geom_leaf;              // the same records in leaf order: the four surfels of level-0 node i at [4 i .. 4 i + 3]
    int32_t ray_width;                    // > 0: rays form rows of this length and a wave takes an 8x8 block of them
    int32_t packets;                      // waves whose rays run together walk the wide hierarchy as one (st_gather_wide)
    StWide wide;
    // the forward's record of what every wave gathered, pass by pass (ids, [slot][lane] like the LDS buffer): the backward replays it
    // instead of walking the hierarchy again.  hdr[0] chunks drawn from the pool, hdr[1] overflow flag (then the backward traces).
    uint32_t *rec_hdr, *rec_chunks, *rec_arena;
    unsigned long long* lone_rec;         // [8][lone_cap][ST_LONE_REC_PASSES][ST_K] sorted (t, id) keys of the rays traced one per wavefront, or nullptr
    uint32_t lone_cap;                    // per region
    uint32_t rec_pool;                    // chunks in the shared pool (behind the n_tiles * ST_REC_STATIC owned ones)
    uint32_t rec_static;                  // n_tiles * ST_REC_STATIC: where the pool starts
    uint32_t n_tiles;                     // waves of the first launch (one 8x8 block of rays each)
    // Both lists are kept per REGION: block b of a launch runs on XCD b % 8 (observed dispatch order -- used for speed only, nothing below is
    // wrong under another placement), the first launch gives XCD x every eighth 64 x 64 patch of the rays (st_tile_of_wave), and what it
    // lists goes to sub-list x, which the second launch hands to the blocks with b % 8 == x again: the waves resident on one XCD at a time
    // trace neighbouring rays and share the subtrees and leaf records their L2 holds (round 5; before, consecutive blocks of four 8x8 ray
    // blocks went round the eight L2s, an XCD's resident waves were spread over half the image and every L2 saw the whole hierarchy:
    // 4.2 GB fetched by the second launch of a C4-size view).
    uint32_t* defer_list;                 // header (ST_LIST_HDR words: ST_CNT / ST_TKT), then [x * defer_cap ..] (tile << 5 | packet): the packets traced by the second launch, one per wave
    uint32_t defer_cap;                   // per region
    uint32_t* lone_list;                  // header, then [x * lone_list_cap ..] indices of the rays that walk alone (behind the per-ray state)
    uint32_t lone_list_cap;               // per region (= the rays of a region: never full)
    uint32_t* lone_slot;                  // [n_rays]: where the first launch listed a ray that walks alone, region << 28 | index in the region's list (written for exactly those rays)
    uint32_t region_blocks;               // blocks of the first launch per region
    float cone, cone_quad, cone_group;    // 1 - cos of the half-angle within which the directions of a block / quadrant / 2x2 group must stay
    const float4* attr;                   // [P][2]: (rgb, others.x) (others.y, -, -, -)
    float bg[3];
    float *rgb, *dpt, *acc, *norm, *dist, *aux, *wet, *state;     // state [n_rays][4]: M2, T_final, hits blended, passes
    const float *g_rgb, *g_dpt, *g_acc, *g_norm, *g_dist, *g_aux;
    float *g_geom, *g_attr, *g_ray_o, *g_ray_d;                   // [P][16], [P][8] (zeroed by the entry point), [n_rays][3] x 2
};

// The surfel records in leaf (= sorted) order: a wide group's 64 candidates are one 4 KB run, the surfel's index rides in the record's
// spare word.
__global__ __launch_bounds__(256) void st_leaf_order_kernel(int n_slots, int P, const uint32_t* __restrict__ perm, const float4* __restrict__ geom,
                                                            float4* __restrict__ geom_leaf)
{
    const int i = blockIdx.x * 256 + threadIdx.x;            // one thread per 16 bytes
    if (i >= n_slots * 4) return;
    const int slot = i >> 2, part = i & 3;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (slot < P) {
        const uint32_t id = perm[slot];
        v = geom[(size_t)id * 4 + part];
        if (part == 3) v.y = __uint_as_float(id);
    }
    geom_leaf[i] = v;
}

// MODE 0: forward (walks, blends, records what it gathered); 1: backward that walks again (no record, or it overflowed);
// 2: backward that replays the forward's record -- same blend arithmetic on the same ids in the same order, no hierarchy.
#ifndef ST_TAB_ENTRIES
#define ST_TAB_ENTRIES 96
#endif
constexpr int ST_TAB = ST_TAB_ENTRIES;                // surfels a wave of the replaying backward accumulates in LDS before its gradients go out
constexpr int ST_TAB_WORDS = ST_TAB * 19; // 18 gradient terms + the surfel's index per entry
constexpr uint32_t ST_REC_DEFERRED = 0xFFFFFFFEu;   // in the last slot of a block's row of the chunk table: its packets went to the second launch

// One 8x8 block of rays (64 consecutive rays when the rays are no image).  only_packet < 0: the first launch -- the block walks as one
// packet if its rays run together; otherwise its packets (quadrants, 2x2 groups) are LISTED for the second launch, one wave each,
// because a wave that walks 16 packets one after the other lasts 16 times as long as its neighbours and the launch as long as that
// wave (measured: total work of 0.2 ms of perfectly spread waves, 3.5 ms launch).  only_packet >= 1: that packet of the block.
template <int MODE>
__device__ __forceinline__ void st_trace_tile(const StArgs& A, const float4* __restrict__ leaf_ro, const float* __restrict__ wide_boxes,
                                              const unsigned long long* __restrict__ wide_vmask, uint32_t (*kb_id)[ST_THREADS],
                                              float (*kb_t)[ST_THREADS], uint32_t* kb_n, uint32_t* tab, int tid, int64_t tile, int only_packet, uint32_t rec_row,
                                              uint32_t region)
{
    constexpr bool BWD = MODE != 0;
    int64_t r = tile * 64 + (tid & 63);
    if (A.ray_width > 0) {                 // 8x8 blocks of neighbouring rays per wave: neighbours walk the same nodes
        const int64_t tiles_x = (A.ray_width + 7) >> 3, rows = A.n_rays / A.ray_width;
        const int64_t px = (tile % tiles_x) * 8 + (tid & 7), py = (tile / tiles_x) * 8 + ((tid >> 3) & 7);
        r = (px < A.ray_width && py < rows) ? py * A.ray_width + px : A.n_rays;
    }
    StProf prof = {0, 0, 0, 0u, 0u};
    prof.begin();
    const bool exists = r < A.n_rays;
    if (!exists) r = 0;                    // the lane stays for the wave-wide steps and neither blends nor writes
    const float ox = A.ray_o[3 * r], oy = A.ray_o[3 * r + 1], oz = A.ray_o[3 * r + 2];
    const float dx = A.ray_d[3 * r], dy = A.ray_d[3 * r + 1], dz = A.ray_d[3 * r + 2];

    float T = 1.0f, C[3] = {0, 0, 0}, D = 0, Aw = 0, N[3] = {0, 0, 0}, X[2] = {0, 0}, dist = 0, M1 = 0, M2 = 0;
    int blended = 0, passes = 0;
    // backward: the upstream gradients, the forward's totals and their contraction
    StRayGrad R = {};
    float Qpre = 0;
    float go[3] = {0, 0, 0}, gdir[3] = {0, 0, 0};
    if (BWD) st_load_ray_grad(A, r, R);

    float prev_t = 0.0f;
    uint32_t prev_id = 0;
    // a ray without a direction (or with a non-finite one) would visit every node: it sees the background
    bool done = !(exists && fabsf(ox) < 1e30f && fabsf(oy) < 1e30f && fabsf(oz) < 1e30f && fabsf(dx) < 1e30f && fabsf(dy) < 1e30f &&
                  fabsf(dz) < 1e30f && (dx != 0.0f || dy != 0.0f || dz != 0.0f));
    const bool no_ray = done;                       // sees the background; written by the first launch
    uint32_t packets_present = 0;
    int packet;
    if (only_packet >= 1) {
        // a listed packet: the first launch found its rays running together (and its block / quadrant not): its rays are the valid rays of
        // its lanes -- no need to repeat the ~200 wave-wide reductions of the assignment for the whole block
        packet = (st_lane_in_packet(A.ray_width > 0, tid & 63, only_packet) && !done) ? only_packet : -1;
    } else {
        packet = st_assign_packets(A, wide_boxes, wide_vmask, !done, tid & 63, ox, oy, oz, dx, dy, dz, packets_present);
    }
    // rays that run with nobody are only listed here; the second launch gives each a wave of its own
    const bool lone = !done && packet < 0;
    bool deferred = false;                          // this block's packets are the second launch's
    uint32_t my_row = rec_row;                      // the row of the chunk table this lane's record lives in
    if (only_packet < 0) {
        const uint32_t dm = packets_present & ~1u;
        if (MODE == 0) {
            const unsigned long long lm = __ballot(lone);
            if (lm) {
                const int first = __builtin_ctzll(lm), lane = tid & 63;
                uint32_t base = 0;
                if (lane == first) base = atomicAdd(&ST_CNT(A.lone_list, region), (uint32_t)__popcll(lm));
                base = (uint32_t)__builtin_amdgcn_readlane((int)base, first);
                if (lone) {
                    const uint32_t at = base + (uint32_t)__popcll(lm & ((1ull << lane) - 1ull));
                    A.lone_list[ST_LIST_HDR + (size_t)region * A.lone_list_cap + at] = (uint32_t)r;
                    A.lone_slot[r] = (region << 28) | at;          // (the replaying backward finds the ray's record from its block's wave)
                }
            }
            if (dm != 0 && A.defer_list != nullptr) {
                const uint32_t cnt = (uint32_t)__popc(dm);
                uint32_t base = 0;
                if ((tid & 63) == 0) base = atomicAdd(&ST_CNT(A.defer_list, region), cnt);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                deferred = base + cnt <= A.defer_cap;                      // else: the region's list is full and the block walks its packets itself
                base += region * A.defer_cap;                              // the item's index over all regions (its row of the chunk table: n_tiles + index)
                if (deferred && (tid & 63) == 0) {
                    uint32_t i = 0;
                    for (uint32_t left = dm; left; left &= left - 1) A.defer_list[ST_LIST_HDR + base + i++] = ((uint32_t)tile << 5) | (uint32_t)__builtin_ctz(left);
                    A.rec_chunks[(size_t)rec_row * ST_REC_PASSES + ST_REC_PASSES - 1] = ST_REC_DEFERRED;
                    A.rec_chunks[(size_t)rec_row * ST_REC_PASSES + ST_REC_PASSES - 2] = base;     // where its packets' rows start (the block's own row holds no record)
                }
            }
        } else {
            deferred = dm != 0 && A.defer_list != nullptr && A.rec_chunks[(size_t)rec_row * ST_REC_PASSES + ST_REC_PASSES - 1] == ST_REC_DEFERRED;
            if (MODE == 2 && deferred) {
                // The replay needs no walk, so nothing ties it to the forward's one-wave-per-packet split: every lane replays ITS packet's
                // record (row n_tiles + first listed item of the block + the packet's rank among the block's packets) and the whole block
                // is one wave again -- 64 busy lanes and one LDS gradient table instead of up to 16 waves of 4-16 rays each.
                const uint32_t base = A.rec_chunks[(size_t)rec_row * ST_REC_PASSES + ST_REC_PASSES - 2];
                if (packet >= 1) my_row = A.n_tiles + base + (uint32_t)__popc(dm & ((1u << packet) - 1u));
                deferred = false;
            }
        }
    } else {
        packets_present = 1u << only_packet;
    }
    const bool mine = only_packet < 0 ? (no_ray || (packet >= 0 && !deferred)) : (packet == only_packet);
    // The replaying backward also takes its block's single rays along when their recorded hits suffice (round 5): the lane follows the
    // ray's own record (the sorted keys st_trace_lone_rays kept) through the same blend loop and the same LDS gradient table as its
    // neighbours, who meet the same surfels.  A wave per such ray (or per four of them) sent 18 float atomics
    // per hit straight to memory: 12 300 rays cost 0.15 ms at C3 size, 52 000 cost 0.56 ms at C4 size, the atomic unit's rate.
    bool lone_here = false;
    const unsigned long long* lrec = nullptr;
    if (MODE == 2 && only_packet < 0 && lone && A.lone_rec != nullptr) {
        const uint32_t code = A.lone_slot[r], lloc = code & 0x0FFFFFFFu;
        if (lloc < A.lone_cap && A.state[4 * r + 3] <= (float)ST_LONE_REC_PASSES) {
            lone_here = true;
            lrec = A.lone_rec + ((size_t)(code >> 28) * A.lone_cap + lloc) * (ST_LONE_REC_PASSES * ST_K);
        }
    }
    bool want = !done && ((!lone && mine) || lone_here);
    // The replaying backward first collects a surfel's gradient terms in LDS (per wave: ST_TAB entries, open addressing on the surfel's
    // index): the rays of a block meet the same ~100 surfels at different ranks and in different passes, and the global float atomics
    // (18 per hit) are what bounds this kernel.  An entry that finds no place within four probes goes out directly.
    if (MODE == 2) {
        for (int e = tid & 63; e < ST_TAB; e += 64) {
#pragma unroll
            for (int k = 0; k < 18; ++k) tab[e * 19 + k] = 0u;
            tab[e * 19 + 18] = ST_REC_NONE;
        }
        wave_lds_sync();
    }
    for (int pass = 0; pass < ST_MAX_PASSES; ++pass) {
        if (__ballot(want) == 0) break;
        int n = 0;
        if (MODE == 2) {
            if (pass >= ST_REC_PASSES - 1) break;
            const uint32_t chunk = (want && !lone_here) ? A.rec_chunks[(size_t)my_row * ST_REC_PASSES + pass] : ST_REC_NONE;
            const bool has_lone = lone_here && want && pass < ST_LONE_REC_PASSES;
            const bool has = chunk < ST_REC_DEFERRED || has_lone;               // (a lane whose packet recorded no further pass: n = 0 ends it below)
            if (__ballot(has) == 0) break;
            const uint32_t* src = A.rec_arena + (size_t)(chunk < ST_REC_DEFERRED ? chunk : 0u) * (ST_K * 64) + (tid & 63);
            const unsigned long long* lsrc = lrec + (has_lone ? pass * ST_K : 0);
#pragma unroll
            for (int j = 0; j < ST_K; ++j) {
                // (a single ray's record holds (t, id) keys, "none" = all ones: its low word is ST_REC_NONE)
                const uint32_t id = has_lone ? (uint32_t)lsrc[j] : (has ? src[j * 64] : ST_REC_NONE);
                kb_id[j][tid] = id;
                if (id != ST_REC_NONE) n = j + 1;
            }
        } else {
            for (uint32_t left = packets_present; left; left &= left - 1) {          // wave-uniform: one walk per packet
                const int pk = __builtin_ctz(left);
                const bool mine = want && packet == pk;
                const int got = pk == 0
                    ? st_gather_wide(A.wide, wide_boxes, wide_vmask, leaf_ro, kb_id, kb_t, tid, ox, oy, oz, dx, dy, dz, prev_t, prev_id, pass == 0, mine, prof)
                    : st_gather_group(A.wide, wide_boxes, wide_vmask, leaf_ro, kb_id, kb_t, kb_n, tid, pk, A.ray_width > 0, ox, oy, oz, dx, dy, dz, prev_t, prev_id,
                                      pass == 0, mine, prof);
                if (mine) n = got;
            }
        }
        if (MODE == 0 && A.rec_arena != nullptr) {
            // the record of this pass: the wave's own chunks first, then one drawn from the pool (one atomic per wave and late pass)
            uint32_t chunk = ST_REC_NONE;
            if (only_packet < 0 && pass < ST_REC_STATIC) {
                chunk = rec_row * ST_REC_STATIC + pass;
            } else if (pass < ST_REC_PASSES - 1) {
                uint32_t got = 0;
                if ((tid & 63) == 0) got = atomicAdd(A.rec_hdr, 1u);
                got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
                if (got < A.rec_pool) chunk = A.rec_static + got;
            }
            if (chunk != ST_REC_NONE) {
                if ((tid & 63) == 0) A.rec_chunks[(size_t)rec_row * ST_REC_PASSES + pass] = chunk;
                uint32_t* dst = A.rec_arena + (size_t)chunk * (ST_K * 64) + (tid & 63);
#pragma unroll
                for (int j = 0; j < ST_K; ++j) dst[j * 64] = (want && j < n) ? kb_id[j][tid] : ST_REC_NONE;
            } else if ((tid & 63) == 0) {
                A.rec_hdr[1] = 1u;                 // the backward walks again
            }
        }
        if (!want) n = 0;                  // (every lane stays with the wave: the merge below moves data across lanes)
        passes += want ? 1 : 0;
        // The wave steps through its lanes' buffers together (a lane without an entry j idles): in the backward, neighbouring rays
        // mostly hold the SAME surfel at the same rank, and lanes that do merge their 18 gradient terms before the atomics.
        for (int j = 0; j < ST_K; ++j) {
            bool act = j < n && !done;
            if (__ballot(act) == 0) break;
            const uint32_t id = act ? kb_id[j][tid] : 0u;
            const float4* g = A.geom + (size_t)id * 4;
            const float4 g0 = g[0], g1 = g[1], g2 = g[2];
            const float opacity = g[3].x;
            const StHit h = st_hit(g0, g1, g2, opacity, ox, oy, oz, dx, dy, dz);      // same expression, same operands as in the gather
            const float t = MODE == 2 ? h.t : kb_t[j][tid];                           // (the same number)
            const float alpha = h.alpha;
            const float test_T = T * (1.0f - alpha);
            if (act && test_T < 0.0001f) { done = true; act = false; }
            const float w = act ? alpha * T : 0.0f;
            const float4 a0 = A.attr[(size_t)id * 2], a1 = A.attr[(size_t)id * 2 + 1];
            const float sgn = h.den > 0.0f ? -1.0f : 1.0f;                   // the normal faces the ray's origin
            const float nfx = sgn * g2.y, nfy = sgn * g2.z, nfz = sgn * g2.w;
            if (!BWD) {
                if (act) {
                    C[0] += w * a0.x; C[1] += w * a0.y; C[2] += w * a0.z;
                    N[0] += w * nfx; N[1] += w * nfy; N[2] += w * nfz;
                    X[0] += w * a0.w; X[1] += w * a1.x;
                    dist += w * (t * t * Aw + M2 - 2.0f * t * M1);
                    D += w * t; Aw += w; M1 += w * t; M2 += w * t * t;
                    atomicAdd(A.wet + id, w);
                }
            } else {
                float gv[18];
#pragma unroll
                for (int k = 0; k < 18; ++k) gv[k] = 0.0f;
                if (act) {
                    const float q = st_hit_q(R, a0, a1, t, nfx, nfy, nfz);
                    Qpre += w * q;
                    // (the per-hit gradient, written out: must equal the copy in st_trace_lone_rays, see mrgs_surfel_blend.h)
                    const float inv1ma = 1.0f / (1.0f - alpha);
                    const float dalpha = T * q - (R.Qtot - Qpre) * inv1ma - R.fT * R.bgdot * inv1ma;
                    const float dG = opacity * dalpha;                                    // no clamp mask, as backward.cu:411-413
                    const float du = -h.u * h.G * dG, dv = -h.v * h.G * dG;
                    const float ax = g0.w, ay = g1.x, az = g1.y, bx = g1.z, by = g1.w, bz = g2.x, nx = g2.y, ny = g2.z, nz = g2.w;
                    const float px = (ox + t * dx) - g0.x, py = (oy + t * dy) - g0.y, pz = (oz + t * dz) - g0.z;
                    const float dpx = du * ax + dv * bx, dpy = du * ay + dv * by, dpz = du * az + dv * bz;
                    const float dt = w * (R.gd + R.gdist * 2.0f * (t * R.fA - R.fM1)) + (dpx * dx + dpy * dy + dpz * dz);
                    const float dnum = dt / h.den, dden = -dt * t / h.den;
                    gv[0] = -dpx + dnum * nx; gv[1] = -dpy + dnum * ny; gv[2] = -dpz + dnum * nz;
                    gv[3] = du * px; gv[4] = du * py; gv[5] = du * pz;
                    gv[6] = dv * px; gv[7] = dv * py; gv[8] = dv * pz;
                    gv[9] = dnum * (g0.x - ox) + dden * dx + sgn * w * R.gn0;
                    gv[10] = dnum * (g0.y - oy) + dden * dy + sgn * w * R.gn1;
                    gv[11] = dnum * (g0.z - oz) + dden * dz + sgn * w * R.gn2;
                    gv[12] = h.G * dalpha;
                    gv[13] = w * R.gc0; gv[14] = w * R.gc1; gv[15] = w * R.gc2; gv[16] = w * R.gx0; gv[17] = w * R.gx1;
                    go[0] += dpx - dnum * nx; go[1] += dpy - dnum * ny; go[2] += dpz - dnum * nz;
                    gdir[0] += t * dpx + dden * nx; gdir[1] += t * dpy + dden * ny; gdir[2] += t * dpz + dden * nz;
                }
                // merge with the horizontal, then the vertical neighbour of the 8x8 block when both hold the same surfel: the lower
                // lane of a pair carries the sum, the upper one is done (DPP moves: quad_perm [1,0,3,2] = lane ^ 1, [2,3,0,1] = lane ^ 2, row_ror:8 = lane ^ 8).
                // The replay merges BEFORE it collects in LDS what is left: neighbouring rays hold the same surfel at the same rank more
                // often than not, and up to eight lanes adding to one LDS row are eight serialised ds_add_f32 per term.
                bool live = act;
                bool placed = false;
                st_merge_pair<0xB1, 1>(gv, id, live, tid);       // quad_perm [1,0,3,2] = lane ^ 1
                st_merge_pair<0x4E, 2>(gv, id, live, tid);       // quad_perm [2,3,0,1] = lane ^ 2
                st_merge_pair<0x128, 8>(gv, id, live, tid);      // row_ror:8 = lane ^ 8
                // what is left collects in the LDS table (kept a lambda: as a plain block the kernel compiles to another schedule)
                auto collect = [&]() {
                    if (MODE == 2 && live) {
                        int slot = (int)(((id * 2654435761u) >> 16) % (uint32_t)ST_TAB);
                        for (int probe = 0; probe < 4 && !placed; ++probe) {
                            const uint32_t old = atomicCAS(&tab[slot * 19 + 18], ST_REC_NONE, id);
                            if (old == ST_REC_NONE || old == id) placed = true;
                            else slot = slot + 1 == ST_TAB ? 0 : slot + 1;
                        }
                        if (placed) {
                            float* row = reinterpret_cast<float*>(tab) + slot * 19;
#pragma unroll
                            for (int k = 0; k < 18; ++k) atomicAdd(row + k, gv[k]);
                        }
                    }
                };
                collect();
                if (live && !placed) st_add_surfel_grad(A, id, gv);
            }
            if (act) { T = test_T; ++blended; }
        }
        if (n < ST_K || done) want = false;
        if (want && MODE != 2) {
            prev_t = kb_t[ST_K - 1][tid];
            prev_id = kb_id[ST_K - 1][tid];
        }
    }
    if (MODE == 2) {                           // the collected gradients go out: one entry per lane and round
        wave_lds_sync();
        for (int e = tid & 63; e < ST_TAB; e += 64) {
            const uint32_t key = tab[e * 19 + 18];
            if (key != ST_REC_NONE) st_add_surfel_grad(A, key, reinterpret_cast<const float*>(tab) + e * 19);
        }
    }
    if (!exists || !((mine && !lone) || lone_here)) return;
    if (!BWD) {
        st_write_ray(A, r, C[0], C[1], C[2], T, D, Aw, dist, N[0], N[1], N[2], X[0], X[1]);
#ifdef ST_PROFILE
        blended = (int)prof.t_fetch; passes = prof.tests; M2 = (float)(wall_clock64() - prof.t0); T = (float)prof.t_cand;   // 100 MHz ticks
#endif
        reinterpret_cast<float4*>(A.state)[r] = make_float4(M2, T, (float)blended, (float)(packet >= 0 ? -passes : passes));   // sign: walked in a packet
    } else {
        st_write_ray_grad(A, r, go[0], go[1], go[2], gdir[0], gdir[1], gdir[2]);
    }
}

// Wave w of region x of the first launch -> its 8x8 block of rays.  The blocks of rays are grouped into SUPERTILES of ST_SUPER x ST_SUPER
// blocks (4 x 4: 32 x 32 rays, 16 waves), supertile s belongs to region s % 8 and a region walks its supertiles in order: the ~500 waves
// an XCD holds at a time cover ~30 compact patches of the image -- whose mirror rays meet compact parts of the scene -- while every XCD
// gets every eighth patch of the WHOLE image, i.e. an equal share of the work.  Measured on the way (round 5, C4 size, first launch /
// replaying backward in us): eight contiguous bands of the image, one per XCD, 2 270 / -- (a view's rays that hit nothing sit in its
// corners: the launch lasts as long as the band through the middle); supertiles of 16 x 16 blocks 1 682 / 1 550, 8 x 8 1 600 / 1 487,
// 4 x 4 1 582 / 1 388; round 4's round-robin of four-block rows 1 604 / 1 074 (+ 1 003 for the single rays the replay now takes along).
// The fetched bytes fall with the patch size (first launch 1 148 -> 541 MB at 8 x 8); the time follows the balance.  Ray sets that are no
// image: runs of ST_SUPER^2 blocks.
#ifndef ST_SUPER_EDGE
#define ST_SUPER_EDGE 4
#endif
constexpr uint32_t ST_SUPER = ST_SUPER_EDGE;
__host__ __device__ __forceinline__ uint32_t st_supertiles(int64_t n_tiles, int32_t ray_width)
{
    if (ray_width <= 0) return (uint32_t)((n_tiles + ST_SUPER * ST_SUPER - 1) / (ST_SUPER * ST_SUPER));
    const uint32_t tiles_x = (uint32_t)(ray_width + 7) >> 3, tiles_y = (uint32_t)(n_tiles / tiles_x);
    return ((tiles_x + ST_SUPER - 1) / ST_SUPER) * ((tiles_y + ST_SUPER - 1) / ST_SUPER);
}
__device__ __forceinline__ int64_t st_tile_of_wave(const StArgs& A, uint32_t region, uint32_t w)
{
    constexpr uint32_t per = ST_SUPER * ST_SUPER;
    const uint32_t s = (w / per) * 8u + region, t = w % per;
    if (A.ray_width <= 0) {
        const uint64_t tile = (uint64_t)s * per + t;
        return tile < A.n_tiles ? (int64_t)tile : -1;
    }
    const uint32_t tiles_x = (uint32_t)(A.ray_width + 7) >> 3, tiles_y = A.n_tiles / tiles_x;
    const uint32_t sxn = (tiles_x + ST_SUPER - 1) / ST_SUPER;
    const uint32_t sy = s / sxn, sx = s - sy * sxn;
    const uint32_t ty = sy * ST_SUPER + t / ST_SUPER, tx = sx * ST_SUPER + t % ST_SUPER;
    if (tx >= tiles_x || ty >= tiles_y) return -1;
    return (int64_t)ty * tiles_x + tx;
}

// first launch: one wave per block of rays.  MODE 0: forward (walks, blends, records what it gathered); 1: backward that walks again
// (no record, or it overflowed); 2: backward that replays the forward's record -- same blend arithmetic on the same ids in the same
// order, no hierarchy.
template <int MODE>
__global__ __launch_bounds__(ST_THREADS) __attribute__((amdgpu_waves_per_eu(MODE == 2 ? 3 : ST_FWD_WAVES, 8))) void st_trace_kernel(StArgs A, const float4* __restrict__ leaf_ro, const float* __restrict__ wide_boxes,
                                                              const unsigned long long* __restrict__ wide_vmask)
{
    __shared__ uint32_t kb_id[ST_K][ST_THREADS];
    __shared__ float kb_t[MODE == 2 ? 1 : ST_K][ST_THREADS];                 // (the replay needs no depths: it recomputes them)
    __shared__ uint32_t kb_n[MODE == 2 ? 1 : ST_THREADS];
    __shared__ uint32_t tab[MODE == 2 ? ST_THREADS / 64 : 1][MODE == 2 ? ST_TAB_WORDS : 1];
    if (MODE != 0 && A.rec_hdr != nullptr && ((A.rec_hdr[1] != 0u) != (MODE == 1))) return;     // the other backward does the work
    const int tid = threadIdx.x;
    // XCD b % 8 takes every eighth supertile of the ray set (st_tile_of_wave)
    const uint32_t region = blockIdx.x & 7u;
    const int64_t tile = st_tile_of_wave(A, region, (blockIdx.x >> 3) * (ST_THREADS / 64) + (tid >> 6));
    if (tile < 0) return;
    st_trace_tile<MODE>(A, leaf_ro, wide_boxes, wide_vmask, kb_id, kb_t, kb_n, tab[MODE == 2 ? tid >> 6 : 0], tid, tile, -1, (uint32_t)tile, region);
}

// ---- rays that run with nobody: one WAVE per ray --------------------------------------------------------------------------------
// A ray whose 2x2 neighbours point elsewhere (silhouettes, normals of barely covered pixels) cannot share a walk.  Walking alone in
// a lane is the slow way on this machine: every step is a dependent ~1 us gather and the wave lasts as long as its slowest lane
// (measured: 4-10 ms for a wave of such lanes, the whole kernel's duration).  So the main kernel only LISTS these rays and this
// kernel gives each of them a wave, with the parallelism turned sideways: the 64 lanes are the 64 children of a wide node, then the
// 64 surfels of a leaf group -- each lane tests ITS surfel against the one ray.  The ray's 16 nearest hits live in lanes 0..15
// (sorted); new hits are merged by rank (rank = entries in front of me, counted with one v_readlane sweep over the other side);
// blending is lane-parallel too: transmittance and the running sums are 16-lane scans, the pixel sums wave reductions, every hit's
// gradient is written by its own lane.

template <bool BWD>
__device__ __forceinline__ void st_trace_lone_rays(const StArgs& A, const float4* __restrict__ leaf, const float* __restrict__ boxes,
                                                   const unsigned long long* __restrict__ vmask, const uint32_t* __restrict__ lone_list,
                                                   unsigned long long* slot, int lane, uint32_t region, uint32_t first_item, uint32_t item_stride,
                                                   bool skip_replayable = false)
{
    // item_stride == 0: the one item `first_item` (the forward's second launch hands items out by ticket); otherwise every item_stride-th
    // skip_replayable (backward): rays whose recorded hits suffice are replayed by their blocks' waves (st_trace_tile)
    const uint32_t listed = ST_CNT(lone_list, region);
    const uint32_t count = listed < A.lone_list_cap ? listed : A.lone_list_cap;
    const StWide& W = A.wide;
    for (uint32_t item = first_item; item < count; item += item_stride) {
        const int64_t r = lone_list[ST_LIST_HDR + (size_t)region * A.lone_list_cap + item];
        if (BWD && skip_replayable && A.lone_rec != nullptr && item < A.lone_cap && A.state[4 * r + 3] <= (float)ST_LONE_REC_PASSES) continue;
        const float ox = A.ray_o[3 * r], oy = A.ray_o[3 * r + 1], oz = A.ray_o[3 * r + 2];
        const float dx = A.ray_d[3 * r], dy = A.ray_d[3 * r + 1], dz = A.ray_d[3 * r + 2];
        const float ivx = 1.0f / dx, ivy = 1.0f / dy, ivz = 1.0f / dz;
        // running totals (uniform) and, for the backward, the forward's totals
        float T = 1.0f, C0 = 0, C1 = 0, C2 = 0, D = 0, Aw = 0, N0 = 0, N1 = 0, N2 = 0, X0 = 0, X1 = 0, dist = 0, M1 = 0, M2 = 0;
        int blended = 0, passes = 0;
        StRayGrad R = {};
        float Qpre = 0;
        float go0 = 0, go1 = 0, go2 = 0, gv0 = 0, gv1 = 0, gv2 = 0;         // per lane partial sums of the ray's own gradient
        if (BWD) st_load_ray_grad(A, r, R);
        unsigned long long prev_key = 0;
        bool done = false;
        // the forward keeps the sorted hits of the first ST_LONE_REC_PASSES passes of every listed ray (128 bytes a pass); a backward whose
        // ray needed no more than that replays them instead of walking the hierarchy again (the walk was 0.3 of the backward's 0.9 ms)
        unsigned long long* rec = (A.lone_rec != nullptr && item < A.lone_cap) ? A.lone_rec + ((size_t)region * A.lone_cap + item) * (ST_LONE_REC_PASSES * ST_K) : nullptr;
        const bool replay = BWD && rec != nullptr && A.state[4 * r + 3] <= (float)ST_LONE_REC_PASSES;
        for (int pass = 0; pass < ST_MAX_PASSES && !done; ++pass) {
            // ---- gather: the ST_K smallest keys above prev_key, sorted, one per lane 0..ST_K-1 ----
            unsigned long long mine = ~0ull;                                   // lanes >= nb hold "none"
            int nb = 0;
            float t_far = INFINITY;
            if (replay) {
                if (lane < ST_K) mine = rec[pass * ST_K + lane];
                nb = (int)__popcll(__ballot(mine != ~0ull));
            } else {
            unsigned long long mask[SW_MAX_LEVELS] = {0, 0, 0, 0};
            int node[SW_MAX_LEVELS] = {0, 0, 0, 0};
            float near1 = 0.f, near2 = 0.f, near3 = 0.f;
            const float prev_t = __uint_as_float((uint32_t)(prev_key >> 32));
            int l = W.n - 1;
            bool fresh = true;
            for (;;) {
                if (fresh) {
                    const int nd = W.off[l] + node[l];
                    fresh = false;
                    if (l > 0) {
                        const float* bx = boxes + (size_t)nd * 384 + lane;
                        const float ax = (bx[0] - ox) * ivx, bxx = (bx[192] - ox) * ivx, ay = (bx[64] - oy) * ivy, by = (bx[256] - oy) * ivy;
                        const float az = (bx[128] - oz) * ivz, bz = (bx[320] - oz) * ivz;
                        const float t_in = fmaxf(fmaxf(fminf(ax, bxx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
                        const float t_out = fminf(fminf(fmaxf(ax, bxx), fmaxf(ay, by)), fmaxf(az, bz));
                        const bool h = t_in <= t_out * 1.00001f + 1e-30f && t_in * 0.99999f <= t_far && t_out * 1.00001f + 1e-30f >= prev_t;
                        mask[l] = __ballot(h) & vmask[nd];
                        if (l == 1) near1 = t_in; else if (l == 2) near2 = t_in; else near3 = t_in;
                    } else {
                        // 64 surfels against the ray at once
                        const float4* g = leaf + ((size_t)node[0] * 64 + lane) * 4;
                        const float4 g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
                        const StHit h = st_hit(g0, g1, g2, g3.x, ox, oy, oz, dx, dy, dz);
                        const unsigned long long cand = ((unsigned long long)__float_as_uint(h.t) << 32) | __float_as_uint(g3.y);
                        const unsigned long long kth = readlane_u64(mine, ST_K - 1);
                        const bool c_ok = ((vmask[nd] >> lane) & 1ull) && h.ok && (pass == 0 || cand > prev_key) && cand < kth;
                        const unsigned long long cmask = __ballot(c_ok);
                        if (cmask) {
                            // new rank of every item: buffer entries keep their order, candidates slot in by key
                            int rank_b = lane;                                 // for lanes < nb
                            int rank_c = 0;
                            for (unsigned long long m = cmask; m; m &= m - 1) {
                                const unsigned long long k = readlane_u64(cand, __builtin_ctzll(m));
                                rank_b += k < mine ? 1 : 0;
                                rank_c += k < cand ? 1 : 0;
                            }
                            for (int j = 0; j < nb; ++j) rank_c += readlane_u64(mine, j) < cand ? 1 : 0;
                            if (lane < ST_K) slot[lane] = ~0ull;
                            wave_lds_sync();
                            if (lane < nb && rank_b < ST_K) slot[rank_b] = mine;
                            if (c_ok && rank_c < ST_K) slot[rank_c] = cand;
                            wave_lds_sync();
                            mine = lane < ST_K ? slot[lane] : ~0ull;
                            nb = min(ST_K, nb + (int)__popcll(cmask));
                            if (nb == ST_K) t_far = __uint_as_float((uint32_t)(readlane_u64(mine, ST_K - 1) >> 32)) * 1.00001f + 1e-30f;
                        }
                        mask[0] = 0;
                    }
                }
                if (mask[l] == 0) {
                    if (l == W.n - 1) break;
                    ++l;
                    continue;
                }
                const float my_near = l == 1 ? near1 : l == 2 ? near2 : near3;
                const float key = ((mask[l] >> lane) & 1ull) ? my_near : INFINITY;
                const float nearest = wave_dpp_min(key);
                if (nearest * 0.99999f > t_far) { mask[l] = 0; continue; }
                const int c = __builtin_ctzll(__ballot(key == nearest));
                mask[l] &= ~(1ull << c);
                node[l - 1] = node[l] * 64 + c;
                --l;
                fresh = true;
            }
            if (!BWD && rec != nullptr && pass < ST_LONE_REC_PASSES && lane < ST_K) rec[pass * ST_K + lane] = mine;
            }   // (walk)
            ++passes;
            // ---- blend: hit j in lane j ----
            const bool has = lane < nb;
            const uint32_t id = (uint32_t)mine;
            const float t = has ? __uint_as_float((uint32_t)(mine >> 32)) : 0.0f;      // "none" is all ones: a NaN as a float
            float4 g0 = make_float4(0, 0, 0, 0), g1 = g0, g2 = g0, a0 = g0, a1 = g0;
            float opacity = 0.f;
            StHit h;
            h.alpha = 0.f; h.den = 1.f; h.u = h.v = h.G = 0.f;
            if (has) {
                const float4* g = A.geom + (size_t)id * 4;
                g0 = g[0]; g1 = g[1]; g2 = g[2]; opacity = g[3].x;
                a0 = A.attr[(size_t)id * 2]; a1 = A.attr[(size_t)id * 2 + 1];
                h = st_hit(g0, g1, g2, opacity, ox, oy, oz, dx, dy, dz);
            }
            const float alpha = has ? h.alpha : 0.0f;
            const float Tj = T * scan16_mul_excl(1.0f - alpha, lane);          // transmittance in front of hit j
            const unsigned long long stop = __ballot(has && Tj * (1.0f - alpha) < 0.0001f);
            const int n_bl = stop ? min(nb, (int)__builtin_ctzll(stop)) : nb;
            const bool bl = lane < n_bl;
            const float w = bl ? alpha * Tj : 0.0f;
            const float sgn = h.den > 0.0f ? -1.0f : 1.0f;
            const float nfx = sgn * g2.y, nfy = sgn * g2.z, nfz = sgn * g2.w;
            const float Ab = Aw + scan16_add_excl(w, lane), M1b = M1 + scan16_add_excl(w * t, lane), M2b = M2 + scan16_add_excl(w * t * t, lane);
            if (!BWD) {
                C0 += wave_dpp_sum(w * a0.x); C1 += wave_dpp_sum(w * a0.y); C2 += wave_dpp_sum(w * a0.z);
                N0 += wave_dpp_sum(w * nfx); N1 += wave_dpp_sum(w * nfy); N2 += wave_dpp_sum(w * nfz);
                X0 += wave_dpp_sum(w * a0.w); X1 += wave_dpp_sum(w * a1.x);
                dist += wave_dpp_sum(w * (t * t * Ab + M2b - 2.0f * t * M1b));
                if (bl) atomicAdd(A.wet + id, w);
            } else {
                const float q = st_hit_q(R, a0, a1, t, nfx, nfy, nfz);
                const float wq = w * q;
                const float Qin = Qpre + scan16_add_excl(wq, lane) + wq;            // inclusive
                if (bl) {       // (the per-hit gradient, written out: must equal the copy in st_trace_tile)
                    const float inv1ma = 1.0f / (1.0f - alpha);
                    const float dalpha = Tj * q - (R.Qtot - Qin) * inv1ma - R.fT * R.bgdot * inv1ma;
                    const float dG = opacity * dalpha;
                    const float du = -h.u * h.G * dG, dv = -h.v * h.G * dG;
                    const float ax = g0.w, ay = g1.x, az = g1.y, bx = g1.z, by = g1.w, bz = g2.x, nx = g2.y, ny = g2.z, nz = g2.w;
                    const float px = (ox + t * dx) - g0.x, py = (oy + t * dy) - g0.y, pz = (oz + t * dz) - g0.z;
                    const float dpx = du * ax + dv * bx, dpy = du * ay + dv * by, dpz = du * az + dv * bz;
                    const float dt = w * (R.gd + R.gdist * 2.0f * (t * R.fA - R.fM1)) + (dpx * dx + dpy * dy + dpz * dz);
                    const float dnum = dt / h.den, dden = -dt * t / h.den;
                    float* gg = A.g_geom + (size_t)id * 16;
                    atomicAdd(gg + 0, -dpx + dnum * nx); atomicAdd(gg + 1, -dpy + dnum * ny); atomicAdd(gg + 2, -dpz + dnum * nz);
                    atomicAdd(gg + 3, du * px); atomicAdd(gg + 4, du * py); atomicAdd(gg + 5, du * pz);
                    atomicAdd(gg + 6, dv * px); atomicAdd(gg + 7, dv * py); atomicAdd(gg + 8, dv * pz);
                    atomicAdd(gg + 9, dnum * (g0.x - ox) + dden * dx + sgn * w * R.gn0);
                    atomicAdd(gg + 10, dnum * (g0.y - oy) + dden * dy + sgn * w * R.gn1);
                    atomicAdd(gg + 11, dnum * (g0.z - oz) + dden * dz + sgn * w * R.gn2);
                    atomicAdd(gg + 12, h.G * dalpha);
                    float* ga_ = A.g_attr + (size_t)id * 8;
                    atomicAdd(ga_ + 0, w * R.gc0); atomicAdd(ga_ + 1, w * R.gc1); atomicAdd(ga_ + 2, w * R.gc2);
                    atomicAdd(ga_ + 3, w * R.gx0); atomicAdd(ga_ + 4, w * R.gx1);
                    go0 += dpx - dnum * nx; go1 += dpy - dnum * ny; go2 += dpz - dnum * nz;
                    gv0 += t * dpx + dden * nx; gv1 += t * dpy + dden * ny; gv2 += t * dpz + dden * nz;
                }
                Qpre += wave_dpp_sum(wq);
            }
            D += wave_dpp_sum(w * t);
            const float sw = wave_dpp_sum(w);
            Aw += sw; M1 += wave_dpp_sum(w * t); M2 += wave_dpp_sum(w * t * t);
            // transmittance behind the blended hits
            const float keep = bl ? 1.0f - alpha : 1.0f;
            float prod = keep;          // product over the row's 16 lanes: inside the quads, then the neighbouring quads by rotation
            prod *= MRGS_DPP(1.0f, prod, 0xb1, 0xf); prod *= MRGS_DPP(1.0f, prod, 0x4e, 0xf); prod *= MRGS_DPP(1.0f, prod, 0x124, 0xf); prod *= MRGS_DPP(1.0f, prod, 0x128, 0xf);
            T *= st_uniform(prod);
            blended += n_bl;
            if (stop || nb < ST_K) done = true;
            else prev_key = readlane_u64(mine, ST_K - 1);
        }
        if (!BWD) {
            if (lane == 0) {
                st_write_ray(A, r, C0, C1, C2, T, D, Aw, dist, N0, N1, N2, X0, X1);
                reinterpret_cast<float4*>(A.state)[r] = make_float4(M2, T, (float)blended, (float)passes);
            }
        } else {
            const float s0 = wave_dpp_sum(go0), s1 = wave_dpp_sum(go1), s2 = wave_dpp_sum(go2), v0 = wave_dpp_sum(gv0), v1 = wave_dpp_sum(gv1), v2 = wave_dpp_sum(gv2);
            if (lane == 0) st_write_ray_grad(A, r, s0, s1, s2, v0, v1, v2);
        }
        if (item_stride == 0u) break;
    }
}

// second launch: every listed packet and every listed single ray gets a wave.  One launch for both: each kind ends in a tail of a few long
// waves, and the two tails overlap instead of following each other.
// FORWARD (MODE 0): ST_REST_BLOCKS blocks of persistent waves.  A wave of XCD x (block b, x = b % 8) takes the next packet of region x's
// list by ticket -- what the first launch's waves on that XCD listed, front to back, so that the waves an XCD holds at a time trace
// neighbouring rays (StArgs) --, and when that list is exhausted it goes on with the lists of the other regions, then with the single rays
// the same way.  The lists of the regions differ: what gets listed are silhouettes and grazing normals, which sit in a few dozen of an
// 800 x 800 view's 169 supertiles, and a static "XCD x walks list x" ran 40 % longer than the region-blind stride of round 4 while
// fetching a third of its bytes (measured, round 5) -- with the tickets the XCDs that finish early take over the tail of the others.
// A ticket is one L2 atomic per ~150 us walk.  BACKWARD (MODE 1 / 2): no walk to keep local (the replay reads records), and the state
// is not the backward's to write: every list is strided over all waves of the launch.
constexpr int ST_REST_BLOCKS = 2048;

// ST_CNT(hdr, r): counts of the eight region lists (final: written by the launch before); ST_TKT(hdr, r): tickets (zeroed by st_init_kernel).  `k`:
// regions this wave has found exhausted (tickets only grow: they stay exhausted).  Wave-uniform result.
__device__ __forceinline__ bool st_next_item(uint32_t* hdr, uint32_t cap, uint32_t own, int lane, uint32_t& k, uint32_t& region, uint32_t& local)
{
    for (; k < 8u; ++k) {
        const uint32_t r = (own + k) & 7u;
        const uint32_t listed = ST_CNT(hdr, r);
        const uint32_t n = listed < cap ? listed : cap;
        uint32_t t = n;
        if (lane == 0) t = atomicAdd(ST_TKT(hdr, r), 1u);      // (no look before the leap: a ticket beyond the end costs one atomic, a look costs one per item)
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t < n) { region = r; local = t; return true; }
    }
    return false;
}

template <int MODE>
__global__ __launch_bounds__(ST_THREADS) __attribute__((amdgpu_waves_per_eu(MODE == 2 ? 3 : ST_FWD_WAVES, 8))) void st_trace_rest_kernel(StArgs A, const float4* __restrict__ leaf_ro, const float* __restrict__ wide_boxes,
                                                                   const unsigned long long* __restrict__ wide_vmask, uint32_t* __restrict__ lone_list)
{
    __shared__ uint32_t kb_id[ST_K][ST_THREADS];
    __shared__ float kb_t[MODE == 2 ? 1 : ST_K][ST_THREADS];
    __shared__ uint32_t kb_n[MODE == 2 ? 1 : ST_THREADS];
    __shared__ uint32_t tab[MODE == 2 ? ST_THREADS / 64 : 1][MODE == 2 ? ST_TAB_WORDS : 1];
    __shared__ unsigned long long slot[ST_THREADS / 64][ST_K];
    if (MODE != 0 && A.rec_hdr != nullptr && ((A.rec_hdr[1] != 0u) != (MODE == 1))) return;     // the other backward does the work
    const int tid = threadIdx.x, lane = tid & 63;
    if (MODE == 0) {
        const uint32_t own = blockIdx.x & 7u;
        uint32_t k = 0, region = 0, local = 0;
        if (A.defer_list != nullptr) {
            while (st_next_item(A.defer_list, A.defer_cap, own, lane, k, region, local)) {
                const uint32_t item = region * A.defer_cap + local;
                const uint32_t code = A.defer_list[ST_LIST_HDR + item];
                if (code == ST_REC_NONE) continue;                 // a slot of a block that found the list full
                st_trace_tile<MODE>(A, leaf_ro, wide_boxes, wide_vmask, kb_id, kb_t, kb_n, tab[0], tid, (int64_t)(code >> 5), (int)(code & 31u), A.n_tiles + item, region);
            }
        }
        k = 0;
        while (st_next_item(lone_list, A.lone_list_cap, own, lane, k, region, local))
            st_trace_lone_rays<false>(A, leaf_ro, wide_boxes, wide_vmask, lone_list, slot[tid >> 6], lane, region, local, 0u);
        return;
    }
    // every stride-th item of the eight lists laid end to end: region r's items start at the sum of the counts before it
    const uint32_t wave = blockIdx.x * (ST_THREADS / 64) + (tid >> 6), stride = gridDim.x * (ST_THREADS / 64);
    if (MODE != 2 && A.defer_list != nullptr) {                    // (MODE 2: the replay of listed packets rides in their blocks' waves of the first launch)
        uint32_t before = 0;
        for (uint32_t region = 0; region < 8u; ++region) {
            const uint32_t listed = ST_CNT(A.defer_list, region);
            const uint32_t count = listed < A.defer_cap ? listed : A.defer_cap;
            for (uint32_t local = (wave + stride - before % stride) % stride; local < count; local += stride) {
                const uint32_t item = region * A.defer_cap + local;
                const uint32_t code = A.defer_list[ST_LIST_HDR + item];
                if (code == ST_REC_NONE) continue;
                st_trace_tile<MODE>(A, leaf_ro, wide_boxes, wide_vmask, kb_id, kb_t, kb_n, tab[MODE == 2 ? tid >> 6 : 0], tid, (int64_t)(code >> 5), (int)(code & 31u), A.n_tiles + item,
                                    region);
            }
            before += count;
        }
    }
    uint32_t before = 0;
    for (uint32_t region = 0; region < 8u; ++region) {
        const uint32_t listed = ST_CNT(lone_list, region);
        st_trace_lone_rays<MODE != 0>(A, leaf_ro, wide_boxes, wide_vmask, lone_list, slot[tid >> 6], lane, region, (wave + stride - before % stride) % stride, stride,
                                      MODE == 2);
        before += listed < A.lone_list_cap ? listed : A.lone_list_cap;
    }
}

}   // namespace

extern "C" {

struct StateLayout { int64_t grid, n_tiles; size_t lone_slot, lone, defer, rec_hdr, rec_chunks, rec_arena, lone_rec, total; uint32_t pool, defer_cap, lone_cap, lone_list_cap, region_blocks; };

// rays form rows only when their number is a whole number of rows: the row length the tracer works with, or 0
static int32_t st_row_width(int64_t n_rays, int32_t ray_width) { return (ray_width > 0 && n_rays % ray_width == 0) ? ray_width : 0; }

static StateLayout st_state(int64_t n_rays, int32_t ray_width)      // in 4-byte words; ray_width as the caller gave it
{
    StateLayout L;
    ray_width = st_row_width(n_rays, ray_width);
    L.n_tiles = (n_rays + 63) / 64;
    if (ray_width > 0) L.n_tiles = (int64_t)((ray_width + 7) / 8) * ((n_rays / ray_width + 7) / 8);
    // eight regions (StArgs): the first launch is region_blocks blocks per region (whole supertiles), every list has a part per region
    L.region_blocks = ((st_supertiles(L.n_tiles, ray_width) + 7u) / 8u) * (ST_SUPER * ST_SUPER * 64u / ST_THREADS);
    L.grid = 8 * (int64_t)L.region_blocks;
    L.defer_cap = (uint32_t)((4 * L.n_tiles + 1024 + 7) / 8);       // per region
    L.pool = (uint32_t)(3 * L.n_tiles + 64);
    L.lone_list_cap = (uint32_t)(n_rays < (int64_t)L.region_blocks * ST_THREADS ? n_rays : (int64_t)L.region_blocks * ST_THREADS);   // per region: every ray of the region
    L.lone_slot = (size_t)4 * n_rays;                                // per ray: where a ray that walks alone was listed
    L.lone = L.lone_slot + (((size_t)n_rays + 63) & ~(size_t)63);                                     // header (counts and tickets per region), ray indices region by region
    L.defer = L.lone + ST_LIST_HDR + (size_t)8 * L.lone_list_cap;             // header, packets of the second launch region by region
    L.rec_hdr = L.defer + ST_LIST_HDR + (size_t)8 * L.defer_cap;
    L.rec_chunks = L.rec_hdr + 16;                                   // one row per block of rays, then one per listed packet
    L.rec_arena = L.rec_chunks + ((size_t)L.n_tiles + (size_t)8 * L.defer_cap) * ST_REC_PASSES;
    L.lone_rec = (L.rec_arena + ((size_t)L.n_tiles * ST_REC_STATIC + L.pool) * (ST_K * 64) + 1) & ~(size_t)1;      // 8-byte keys
    L.lone_cap = (uint32_t)((ST_LONE_CAP_TILES * L.n_tiles + 1024 + 7) / 8);        // per region
    L.total = L.lone_rec + (size_t)8 * L.lone_cap * ST_LONE_REC_PASSES * ST_K * 2;
    return L;
}

size_t mrgs_surfel_trace_state_floats(int64_t n_rays, int32_t ray_width) { return n_rays < 0 ? 0 : st_state(n_rays, ray_width).total; }
size_t mrgs_surfel_trace_state_floats_norecord(int64_t n_rays, int32_t ray_width) { return n_rays < 0 ? 0 : st_state(n_rays, ray_width).rec_arena; }

// Introspection for the tests: word offsets inside `state` of [0] the lists of rays traced one per wavefront (their counts per
// region at a stride of 64 words), [1] the lists of packets handed to the second launch (counts the same way), [2] the record header (word 0: chunks taken from the shared
// pool, word 1: non-zero = the record overflowed / was not kept and the backward walks again), [3] the replay record, [4] the full size.
int mrgs_surfel_trace_state_layout(int64_t n_rays, int32_t ray_width, size_t* offsets5)
{
    if (n_rays < 0 || !offsets5) return MRGS_E_BAD_ARG;
    const StateLayout L = st_state(n_rays, ray_width);
    offsets5[0] = L.lone; offsets5[1] = L.defer; offsets5[2] = L.rec_hdr; offsets5[3] = L.rec_arena; offsets5[4] = L.total;
    return MRGS_OK;
}

// rays and blocks of rays are carried in 32-bit words (ray indices in the lists, `tile << 5 | packet` codes, the launch grid)
static bool st_ray_count_supported(int64_t n_rays, int32_t ray_width)
{
    if (n_rays >= ((int64_t)1 << 31)) return false;
    return st_state(n_rays, ray_width).n_tiles < ((int64_t)1 << 27);
}

__global__ void st_fill_bg_kernel(int64_t n_rays, float b0, float b1, float b2, float* __restrict__ rgb)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rays) { rgb[3 * i] = b0; rgb[3 * i + 1] = b1; rgb[3 * i + 2] = b2; }
}

// start-of-trace initialisation in one launch (see st_launch): `defer` = header (16 words) + list, directly followed by the record header
// (16 words) and the chunk table -- n_ff words from the list's start are set to all ones, then the three headers are written
__global__ __launch_bounds__(256) void st_init_kernel(uint32_t* __restrict__ lone_hdr, uint32_t* __restrict__ defer_hdr, uint32_t* __restrict__ rec_hdr,
                                                      size_t n_ff, uint32_t rec_flag, float* __restrict__ wet, size_t n_wet)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t* ff = defer_hdr + ST_LIST_HDR;
    // (rec_hdr lies inside [ff, ff + n_ff): its 16 words are written by the threads that own them, with the header's values)
    if (i < n_ff) {
        uint32_t* w = ff + i;
        uint32_t v = 0xFFFFFFFFu;
        if (w >= rec_hdr && w < rec_hdr + 16) v = (w == rec_hdr + 1) ? rec_flag : 0u;
        *w = v;
    }
    if (i < (size_t)ST_LIST_HDR) { lone_hdr[i] = 0u; defer_hdr[i] = 0u; }
    if (i < n_wet && wet != nullptr) wet[i] = 0.0f;
}

__global__ __launch_bounds__(256) void st_zero2_kernel(float4* __restrict__ a, size_t na, float4* __restrict__ b, size_t nb)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < na) a[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nb) b[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// 1 - cos of the half-angle within which a block / quadrant / 2x2 group of rays must stay to share a walk (st_run_together)
constexpr float ST_CONE = 0.005f;
constexpr float ST_CONE_QUAD = ST_CONE;
constexpr float ST_CONE_GROUP = 0.2f * ST_CONE;     // 2x2 groups must be tighter still: four rays rarely pay for a wide beam

static int st_launch(bool bwd, void* blob, int64_t n_surfels, int64_t n_rays, int32_t ray_width, size_t state_floats, StArgs& a, hipStream_t st)
{
    a.n_rays = n_rays;
    const BlobLayout bl = st_blob(n_surfels);
    float4* leaf = (float4*)((char*)blob + bl.leaf);
    a.geom_leaf = leaf;
    a.wide = st_wide(n_surfels);
    const float* wide_boxes = (const float*)((char*)blob + bl.wide_boxes);
    const unsigned long long* wide_vmask = (const unsigned long long*)((char*)blob + bl.wide_vmask);
    hipLaunchKernelGGL(st_leaf_order_kernel, dim3((bl.n_slots * 4 + 255) / 256), dim3(256), 0, st, bl.n_slots, (int)n_surfels,
                       (const uint32_t*)((char*)blob + bl.perm), a.geom, leaf);
    a.ray_width = st_row_width(n_rays, ray_width);
    static const bool no_packets = getenv("MRGS_TRACE_NO_PACKETS") != nullptr;      // developer switch: every ray gets a wave of its own
    a.packets = no_packets ? 0 : 1;
    a.cone = ST_CONE;
    a.cone_quad = ST_CONE_QUAD;
    a.cone_group = ST_CONE_GROUP;
    const StateLayout SL = st_state(n_rays, ray_width);
    if (state_floats < SL.rec_arena) return MRGS_E_WORKSPACE;
    const bool have_arena = state_floats >= SL.total;       // a state without the replay record (forward-only callers): the backward walks again
    const dim3 grid((unsigned)SL.grid), rgrid(ST_REST_BLOCKS);
    uint32_t* words = reinterpret_cast<uint32_t*>(a.state);
    a.lone_list = words + SL.lone;
    a.lone_slot = words + SL.lone_slot;
    a.defer_list = words + SL.defer;
    a.defer_cap = SL.defer_cap;
    a.lone_list_cap = SL.lone_list_cap;
    a.region_blocks = SL.region_blocks;
    a.rec_hdr = words + SL.rec_hdr;
    a.rec_chunks = words + SL.rec_chunks;
    a.rec_arena = words + SL.rec_arena;
    a.rec_pool = SL.pool;
    a.lone_rec = have_arena ? reinterpret_cast<unsigned long long*>(words + SL.lone_rec) : nullptr;
    a.lone_cap = SL.lone_cap;
    a.rec_static = (uint32_t)(SL.n_tiles * ST_REC_STATIC);
    a.n_tiles = (uint32_t)SL.n_tiles;
    static const bool no_record = getenv("MRGS_TRACE_NO_RECORD") != nullptr;          // developer switch: the backward always walks again
    static const bool no_defer = getenv("MRGS_TRACE_NO_DEFER") != nullptr;            // developer switch: every block walks its own packets
    if (no_defer) a.defer_list = nullptr;
    if (no_record) a.lone_rec = nullptr;
    if (!bwd) {
        // the three list / record headers (zeros), the list of deferred packets and the record's chunk table (all ones), the surfels'
        // `wet` sums (zeros): ONE launch instead of six memsets of 4-5 us each
        const bool keep = !(no_record || !have_arena);
        if (!keep) a.rec_arena = nullptr;
        const size_t n_ff = (size_t)8 * SL.defer_cap + ((size_t)SL.n_tiles + (size_t)8 * SL.defer_cap) * ST_REC_PASSES + 16;   // defer lists .. end of rec_chunks (the header between them is rewritten)
        const size_t n_init = n_ff > (size_t)n_surfels ? n_ff : (size_t)n_surfels;
        hipLaunchKernelGGL(st_init_kernel, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, st, a.lone_list, words + SL.defer, a.rec_hdr, n_ff,
                           keep ? 0u : 0x01010101u, a.wet, (size_t)n_surfels);
        hipLaunchKernelGGL(st_trace_kernel<0>, grid, dim3(ST_THREADS), 0, st, a, a.geom_leaf, wide_boxes, wide_vmask);
        hipLaunchKernelGGL(st_trace_rest_kernel<0>, rgrid, dim3(ST_THREADS), 0, st, a, a.geom_leaf, wide_boxes, wide_vmask, a.lone_list);
    } else {
        // exactly one of the two pairs does the work: the replay of the forward's record, or -- when the record overflowed -- the walk
        hipLaunchKernelGGL(st_trace_kernel<2>, grid, dim3(ST_THREADS), 0, st, a, a.geom_leaf, wide_boxes, wide_vmask);
        hipLaunchKernelGGL(st_trace_rest_kernel<2>, rgrid, dim3(ST_THREADS), 0, st, a, a.geom_leaf, wide_boxes, wide_vmask, a.lone_list);
        hipLaunchKernelGGL(st_trace_kernel<1>, grid, dim3(ST_THREADS), 0, st, a, a.geom_leaf, wide_boxes, wide_vmask);
        hipLaunchKernelGGL(st_trace_rest_kernel<1>, rgrid, dim3(ST_THREADS), 0, st, a, a.geom_leaf, wide_boxes, wide_vmask, a.lone_list);
    }
    return MRGS_LAUNCH_STATUS();
}

// what both directions put into StArgs themselves (st_launch adds everything derived from the blob and the state): the forward writes
// the six per-ray maps, the backward only reads them
static StArgs st_args(const float* ray_o, const float* ray_d, const float* geom, const float* attr, const float* bg_host, const float* rgb, const float* dpt,
                      const float* acc, const float* norm, const float* aux, const float* state)
{
    StArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ray_o = ray_o; a.ray_d = ray_d; a.geom = (const float4*)geom; a.attr = (const float4*)attr;
    a.bg[0] = bg_host[0]; a.bg[1] = bg_host[1]; a.bg[2] = bg_host[2];
    a.rgb = const_cast<float*>(rgb); a.dpt = const_cast<float*>(dpt); a.acc = const_cast<float*>(acc); a.norm = const_cast<float*>(norm);
    a.aux = const_cast<float*>(aux); a.state = const_cast<float*>(state);
    return a;
}

int mrgs_surfel_trace_forward(void* blob, int64_t n_surfels, int64_t n_rays, int32_t ray_width, const float* ray_o, const float* ray_d, const float* geom,
                              const float* attr, const float* bg_host, float* rgb, float* dpt, float* acc, float* norm, float* dist,
                              float* aux, float* wet, float* state, size_t state_floats, void* stream)
{
    if (n_rays < 0 || n_surfels < 0 || n_surfels > (int64_t)1 << 24 || !st_ray_count_supported(n_rays, ray_width)) return MRGS_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (n_rays == 0) {                                                     // nothing traced: every surfel's weight sum is zero
        if (n_surfels > 0 && wet) MRGS_HIP_TRY(hipMemsetAsync(wet, 0, (size_t)n_surfels * 4, st));
        return MRGS_OK;
    }
    if (!bg_host || !rgb || !dpt || !acc || !norm || !dist || !aux) return MRGS_E_BAD_ARG;
    if (n_surfels > 0 && (!ray_o || !ray_d || !state || !blob || !geom || !attr || !wet)) return MRGS_E_BAD_ARG;
    if (n_surfels == 0) {                                                  // nothing to hit: background everywhere
        MRGS_HIP_TRY(hipMemsetAsync(dpt, 0, n_rays * 4, st));
        MRGS_HIP_TRY(hipMemsetAsync(acc, 0, n_rays * 4, st));
        MRGS_HIP_TRY(hipMemsetAsync(norm, 0, n_rays * 12, st));
        MRGS_HIP_TRY(hipMemsetAsync(dist, 0, n_rays * 4, st));
        MRGS_HIP_TRY(hipMemsetAsync(aux, 0, n_rays * 8, st));
        hipLaunchKernelGGL(st_fill_bg_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, n_rays, bg_host[0], bg_host[1], bg_host[2], rgb);
        return MRGS_LAUNCH_STATUS();    // (an empty model, e.g. after pruning everything; `state` is not touched)
    }
    StArgs a = st_args(ray_o, ray_d, geom, attr, bg_host, rgb, dpt, acc, norm, aux, state);
    a.dist = dist; a.wet = wet;
    return st_launch(false, blob, n_surfels, n_rays, ray_width, state_floats, a, st);
}

int mrgs_surfel_trace_backward(void* blob, int64_t n_surfels, int64_t n_rays, int32_t ray_width, const float* ray_o, const float* ray_d, const float* geom,
                               const float* attr, const float* bg_host, const float* rgb, const float* dpt, const float* acc,
                               const float* norm, const float* aux, const float* state, size_t state_floats, const float* g_rgb, const float* g_dpt,
                               const float* g_acc, const float* g_norm, const float* g_dist, const float* g_aux, float* g_geom,
                               float* g_attr, float* g_ray_o, float* g_ray_d, void* stream)
{
    if (n_rays < 0 || n_surfels <= 0 || n_surfels > (int64_t)1 << 24 || !st_ray_count_supported(n_rays, ray_width)) return MRGS_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (!g_geom || !g_attr) return MRGS_E_BAD_ARG;
    if ((((uintptr_t)g_geom | (uintptr_t)g_attr) & 15u) == 0) {                                             // one launch, not two memsets
        hipLaunchKernelGGL(st_zero2_kernel, dim3((unsigned)(((size_t)n_surfels * 4 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<float4*>(g_geom),
                           (size_t)n_surfels * 4, reinterpret_cast<float4*>(g_attr), (size_t)n_surfels * 2);
        if (int rc = MRGS_LAUNCH_STATUS()) return rc;
    } else {
        MRGS_HIP_TRY(hipMemsetAsync(g_geom, 0, (size_t)n_surfels * 64, st));
        MRGS_HIP_TRY(hipMemsetAsync(g_attr, 0, (size_t)n_surfels * 32, st));
    }
    if (n_rays == 0) return MRGS_OK;
    if (!blob || !ray_o || !ray_d || !geom || !attr || !bg_host || !rgb || !dpt || !acc || !norm || !aux || !state || !g_ray_o || !g_ray_d)
        return MRGS_E_BAD_ARG;                                  // (any of the six upstream gradients may be NULL = zeros)
    StArgs a = st_args(ray_o, ray_d, geom, attr, bg_host, rgb, dpt, acc, norm, aux, state);
    a.g_rgb = g_rgb; a.g_dpt = g_dpt; a.g_acc = g_acc; a.g_norm = g_norm; a.g_dist = g_dist; a.g_aux = g_aux;
    a.g_geom = g_geom; a.g_attr = g_attr; a.g_ray_o = g_ray_o; a.g_ray_d = g_ray_d;
    return st_launch(true, blob, n_surfels, n_rays, ray_width, state_floats, a, st);
}

}   // extern "C"
