// mrgs_surfel_trace.h -- what the two translation units of the surfel tracer share: the constants, the shape of the 64-ary hierarchy
// (StWide) and the layout of the blob that holds it (BlobLayout).  mrgs_surfel_hier.hip builds into that blob, mrgs_surfel_trace.hip walks it.
// (An unnamed namespace, like the .hip files': the kernels' names carry StWide's.)
#pragma once
#include <cstring>

#include "mrgs_internal.h"

namespace {

#ifndef ST_FWD_WAVES
#define ST_FWD_WAVES 4                    // waves per SIMD the forward walking kernels are compiled for (register budget 512 / that)
#endif
constexpr int ST_K = 16;                  // hits gathered per pass
constexpr int ST_THREADS = 256;
constexpr int ST_MAX_PASSES = 256;        // 4096 hits per ray at most
constexpr float ST_EXTENT = 3.0f;         // optix_utils.py:44 (3-sigma quad)

constexpr int ST_REC_STATIC = 3;          // chunks of the hit record every wave owns; further passes draw from a shared pool
#ifndef ST_LONE_CAP_TILES
#define ST_LONE_CAP_TILES 8             // rays per block of rays the single rays' record has room for (x n_tiles / 8 per region); 2 was too few: the regions differ by 2x
#endif
#ifndef ST_LONE_PASSES
#define ST_LONE_PASSES 8
#endif
constexpr int ST_LONE_REC_PASSES = ST_LONE_PASSES;   // passes of a ray traced alone whose 16 sorted hits are kept for the backward (more: it walks again)
constexpr int ST_REC_PASSES = 16;         // passes of a wave the record can hold (beyond: the backward traces again)
constexpr uint32_t ST_REC_NONE = 0xFFFFFFFFu;
// Header of the two per-region lists (StArgs::lone_list / defer_list): ST_LIST_HDR words in front of the entries; region r's count sits
// at word 64 r and its ticket (second launch of the forward) at word 64 r + 32 -- every counter in a 128-byte line of its own.  Round 5
// first kept the sixteen words side by side: every listing wave of the first launch and every ticket of the second then met on ONE line
// at the memory-side atomic unit (~11 ns per operation, tools/ubench), and 20 000 tickets of two operations each put 0.4 ms of
// serialised waiting into a 0.6 ms launch (measured: tickets without stealing 1.24 ms against 0.86 ms for computed indices).
constexpr int ST_LIST_HDR = 512;
#define ST_CNT(hdr, r) ((hdr)[64u * (r)])
#define ST_TKT(hdr, r) ((hdr) + 64u * (r) + 32u)
constexpr int SW_MAX_LEVELS = 4;          // 64^4 surfels
struct StWide {
    int32_t n;                            // levels; level 0 holds surfels (sorted position 64 g + c), the root is node 0 of level n-1
    int32_t off[SW_MAX_LEVELS];           // first node of level l
    int32_t cnt[SW_MAX_LEVELS];
    int32_t total;
};

StWide st_wide(int64_t P)
{
    StWide w;
    std::memset(&w, 0, sizeof(w));
    int64_t c = (P + 63) / 64;
    if (c < 1) c = 1;
    int32_t off = 0;
    for (int l = 0; l < SW_MAX_LEVELS; ++l) {
        w.off[l] = off; w.cnt[l] = (int32_t)c; off += (int32_t)c; w.n = l + 1;
        if (c == 1) break;
        c = (c + 63) / 64;
    }
    w.total = off;
    return w;
}

struct BlobLayout { size_t perm, leaf, wide_boxes, wide_vmask, total; int n_slots; };

static BlobLayout st_blob(int64_t n_surfels)          // sorted order | surfel records in that order (filled by the trace calls) | wide boxes | wide masks
{
    const StWide w = st_wide(n_surfels);
    BlobLayout b;
    b.n_slots = 64 * w.cnt[0];
    b.perm = 0;
    b.leaf = mrgs_align_up((size_t)b.n_slots * 4, 256);
    b.wide_boxes = mrgs_align_up(b.leaf + (size_t)b.n_slots * 64, 256);
    b.wide_vmask = mrgs_align_up(b.wide_boxes + (size_t)w.total * 1536, 256);
    b.total = mrgs_align_up(b.wide_vmask + (size_t)w.total * 8, 256);
    return b;
}

}   // namespace
