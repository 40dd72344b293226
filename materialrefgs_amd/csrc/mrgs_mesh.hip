// TSDF fusion, marching tetrahedra and floater removal: the mesh extraction step of the training loops (utils/mesh_utils.py:30-51,
// 127-253, 309-404; contract in include/mrgs.h).
//
// The reference copies every depth map to the host and fuses it with Open3D or with a torch loop that makes ~20 passes over the whole
// sample set per view, extracts with skimage's marching cubes per 512^3 crop, merges vertices by rounding and clusters with Open3D.
// Here:
//   fuse      one thread per sample, neighbouring lanes neighbouring lattice points along the fastest axis; the view loop runs inside the
//             kernel with tsdf and w in registers, the views come from a device table (wave-uniform reads), the field is written once.
//             Algorithmic bytes: 4 per sample written, the depth maps through L2 (their taps are neighbours where the lanes are).
//   attributes  the texturing pass: vertex_fuse_kernel below, a sibling of the fusion with CP channel accumulators per point.
//   count     per slab of planes along the slowest axis, one thread per lattice point: the 7-bit mask of its crossing edges (an edge is
//             owned by its lower end), the triangles of the cube above it, an in-block scan; one word per point, three sums per block,
//             then one workgroup scans the three rows of sums (block_counts_exclusive_scan, mrgs_wave.h) into block offsets and the running totals.  The host reads 16 bytes.
//   emit      the same two launches per slab again (the words are slab-sized, not lattice-sized), then one thread per lattice point
//             writes its vertices and its cube's triangles: a corner's index is base[owner] + popcount(mask[owner] below its kind), so
//             triangles share indices by construction -- no sort, no merge.
//   clusters  lock-free min-label hooking over the triangles (a link always points to the lower vertex index, so the root of a
//             component is its smallest index), pointer jumping over the vertices, per-label triangle counts.
// The tetrahedra are the six Kuhn simplices of a cube, (c, c+e_a, c+e_a+e_b, c+e_a+e_b+e_c) per permutation: corner offsets are nested bit
// sets, an edge's owner is its smaller set and its kind the set difference, and the winding follows from two parities -- no table.
#include "mrgs_internal.h"
#include "mrgs_wave.h"
#include "mrgs_cc.h"

namespace {

constexpr int MESH_BLOCK = 256;                 // lattice points per workgroup, one per thread
constexpr long long MESH_MAX_SLAB_POINTS = 1ll << 28;   // 12 triangles a point still fit the 32-bit slab-local offsets
// word of a lattice point: bits 0-6 mask of crossing edges (bit c-1: direction code c = 4 dx + 2 dy + dz), 7-17 vertices before it in
// its block (<= 7 * 255), 18-29 triangles before it in its block (<= 12 * 255)
__device__ __forceinline__ unsigned word_mask(unsigned w) { return w & 0x7Fu; }
__device__ __forceinline__ unsigned word_vpre(unsigned w) { return (w >> 7) & 0x7FFu; }
__device__ __forceinline__ unsigned word_tpre(unsigned w) { return (w >> 18) & 0xFFFu; }

// ---- fusion ----------------------------------------------------------------------------------------------------------------------
struct FuseArgs {
    int mode, n0, n1, n2, n_views;
    long long n;
    float origin[3], spacing[3], center[3];
    float radius, trunc, depth_trunc;
    const float* points;
};

__global__ __launch_bounds__(256) void tsdf_fuse_kernel(FuseArgs a, const MrgsTsdfView* __restrict__ views, float* __restrict__ field,
                                                        float* __restrict__ weight)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n) return;
    float x, y, z, trunc = a.trunc;
    if (a.mode == MRGS_TSDF_POINTS) {
        x = a.points[3 * idx]; y = a.points[3 * idx + 1]; z = a.points[3 * idx + 2];
    } else {
        const int k = (int)(idx % a.n2);
        const long long r = idx / a.n2;
        const int j = (int)(r % a.n1), i = (int)(r / a.n1);
        x = a.origin[0] + a.spacing[0] * (float)i; y = a.origin[1] + a.spacing[1] * (float)j; z = a.origin[2] + a.spacing[2] * (float)k;
        if (a.mode == MRGS_TSDF_CONTRACTED) {
            const float mag = sqrtf(x * x + y * y + z * z);
            if (mag > 1.0f) trunc = trunc * (1.0f / (2.0f - fminf(mag, 1.9f)));
            if (!(mag < 1.0f)) { const float s = 1.0f / ((2.0f - mag) * mag); x *= s; y *= s; z *= s; }
            x = a.center[0] + a.radius * x; y = a.center[1] + a.radius * y; z = a.center[2] + a.radius * z;
        }
    }
    float tsdf = 1.0f, w = 1.0f;
    for (int v = 0; v < a.n_views; ++v) {
        const MrgsTsdfView& vw = views[v];
        const float* m = vw.proj;
        const float cx = x * m[0] + y * m[4] + z * m[8] + m[12];
        const float cy = x * m[1] + y * m[5] + z * m[9] + m[13];
        const float cw = x * m[3] + y * m[7] + z * m[11] + m[15];
        const float nx = cx / cw, ny = cy / cw;
        const int H = vw.H, W = vw.W;
        if (!(nx > -1.0f && nx < 1.0f && ny > -1.0f && ny < 1.0f && cw > 0.0f) || H < 1 || W < 1) continue;
        // grid_sample, bilinear, align_corners = True, border padding
        const float px = fminf(fmaxf((nx + 1.0f) * 0.5f * (float)(W - 1), 0.0f), (float)(W - 1));
        const float py = fminf(fmaxf((ny + 1.0f) * 0.5f * (float)(H - 1), 0.0f), (float)(H - 1));
        const float fx = floorf(px), fy = floorf(py);
        const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float tx = px - fx, ty = py - fy;
        const float* __restrict__ dm = vw.depth;
        const float d00 = dm[(size_t)y0 * W + x0], d01 = dm[(size_t)y0 * W + x1], d10 = dm[(size_t)y1 * W + x0], d11 = dm[(size_t)y1 * W + x1];
        if (a.depth_trunc > 0.0f) {
            const float lo = fminf(fminf(d00, d01), fminf(d10, d11)), hi = fmaxf(fmaxf(d00, d01), fmaxf(d10, d11));
            if (!(lo > 0.0f && hi <= a.depth_trunc)) continue;
        }
        const float d = d00 * ((1.0f - tx) * (1.0f - ty)) + d01 * (tx * (1.0f - ty)) + d10 * ((1.0f - tx) * ty) + d11 * (tx * ty);
        const float sdf = d - cw;
        if (!(sdf > -trunc)) continue;
        const float t = fminf(fmaxf(sdf / trunc, -1.0f), 1.0f);
        tsdf = (tsdf * w + t) / (w + 1.0f);
        w += 1.0f;
    }
    field[idx] = tsdf;
    if (weight) weight[idx] = w;
}

// ---- vertex attributes -----------------------------------------------------------------------------------------------------------
// The "texturing" pass (compute_unbounded_tsdf(..., return_rgb=True), utils/mesh_utils.py:322-373, called at :402): per point the running
// mean of CP attribute channels over the views that accept it, acceptance exactly tsdf_fuse_kernel's.  One thread per point, the view
// loop inside the kernel with a[CP] and w in registers (CP is a template parameter: the accumulators are never indexed dynamically),
// the table read wave-uniformly, one launch per call.  The maps are channel-last, so a corner is CP / 4 16-byte loads, and those sit
// behind the acceptance branch: a rejected view costs its four depth texels and nothing else.  No atomics, no LDS: bitwise repeatable.
// Mesh vertices arrive ordered by owning lattice point (mrgs_mesh_emit), so neighbouring lanes tap neighbouring texels.
// Algorithmic bytes: 12 read and 4 CP (+ 4) written per point; per accepted (point, view) pair 16 B of depth and 16 CP B of attributes
// pass through L2.
// The map pointers come out of the device table, where the compiler cannot see their address space: named global here, so that the taps
// are global loads with counted waits, not flat ones that wait for everything.
typedef float Float4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float GlobalF;
typedef __attribute__((address_space(1))) Float4 GlobalF4;
struct VertexFuseArgs {
    int n_views;
    long long n;
    float w0, trunc, depth_trunc;
};

// Above CP = 4 the occupancy target is 4 waves per SIMD: at the default target the scheduler keeps 7 by holding the 4 (CP / 4) corner loads
// of a view back to two to four in flight (66-68 VGPRs); with the target lowered it issues all of them before the first use.
template <int CP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, CP > 4 ? 4 : 8)))
void vertex_fuse_kernel(VertexFuseArgs a, const MrgsAttrView* __restrict__ views, const float* __restrict__ points, float* __restrict__ out,
                        float* __restrict__ weight)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n) return;
    const float x = points[3 * idx], y = points[3 * idx + 1], z = points[3 * idx + 2], trunc = a.trunc;
    float acc[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[c] = 0.0f;
    float w = a.w0;
    for (int v = 0; v < a.n_views; ++v) {
        const MrgsAttrView& vw = views[v];
        const float* m = vw.proj;
        const float cx = x * m[0] + y * m[4] + z * m[8] + m[12];
        const float cy = x * m[1] + y * m[5] + z * m[9] + m[13];
        const float cw = x * m[3] + y * m[7] + z * m[11] + m[15];
        const float nx = cx / cw, ny = cy / cw;
        const int H = vw.H, W = vw.W;
        if (!(nx > -1.0f && nx < 1.0f && ny > -1.0f && ny < 1.0f && cw > 0.0f) || H < 1 || W < 1) continue;
        const float px = fminf(fmaxf((nx + 1.0f) * 0.5f * (float)(W - 1), 0.0f), (float)(W - 1));
        const float py = fminf(fmaxf((ny + 1.0f) * 0.5f * (float)(H - 1), 0.0f), (float)(H - 1));
        const float fx = floorf(px), fy = floorf(py);
        const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float tx = px - fx, ty = py - fy;
        const GlobalF* __restrict__ dm = (const GlobalF*)vw.depth;
        const size_t i00 = (size_t)y0 * W + x0, i01 = (size_t)y0 * W + x1, i10 = (size_t)y1 * W + x0, i11 = (size_t)y1 * W + x1;
        const float d00 = dm[i00], d01 = dm[i01], d10 = dm[i10], d11 = dm[i11];
        if (a.depth_trunc > 0.0f) {
            const float lo = fminf(fminf(d00, d01), fminf(d10, d11)), hi = fmaxf(fmaxf(d00, d01), fmaxf(d10, d11));
            if (!(lo > 0.0f && hi <= a.depth_trunc)) continue;
        }
        const float w00 = (1.0f - tx) * (1.0f - ty), w01 = tx * (1.0f - ty), w10 = (1.0f - tx) * ty, w11 = tx * ty;
        const float d = d00 * w00 + d01 * w01 + d10 * w10 + d11 * w11;
        const float sdf = d - cw;
        if (!(sdf > -trunc)) continue;
        const GlobalF4* __restrict__ am = (const GlobalF4*)vw.attr;
        const float wp = w + 1.0f;
        Float4 t00[CP / 4], t01[CP / 4], t10[CP / 4], t11[CP / 4];      // every load of the view before the first use
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
            t00[q] = am[i00 * (CP / 4) + q]; t01[q] = am[i01 * (CP / 4) + q]; t10[q] = am[i10 * (CP / 4) + q]; t11[q] = am[i11 * (CP / 4) + q];
        }
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
            const Float4 a00 = t00[q], a01 = t01[q], a10 = t10[q], a11 = t11[q];
            acc[4 * q] = (acc[4 * q] * w + (a00.x * w00 + a01.x * w01 + a10.x * w10 + a11.x * w11)) / wp;
            acc[4 * q + 1] = (acc[4 * q + 1] * w + (a00.y * w00 + a01.y * w01 + a10.y * w10 + a11.y * w11)) / wp;
            acc[4 * q + 2] = (acc[4 * q + 2] * w + (a00.z * w00 + a01.z * w01 + a10.z * w10 + a11.z * w11)) / wp;
            acc[4 * q + 3] = (acc[4 * q + 3] * w + (a00.w * w00 + a01.w * w01 + a10.w * w10 + a11.w * w11)) / wp;
        }
        w = wp;
    }
    float4* __restrict__ o = (float4*)out + (size_t)idx * (CP / 4);
#pragma unroll
    for (int q = 0; q < CP / 4; ++q) o[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    if (weight) weight[idx] = w;
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------
struct MeshArgs {
    int n0, n1, n2;
    int p0, cubes_end, own_end;     // the slab's first plane; its cubes sit in planes [p0, cubes_end); it owns the vertices of [p0, own_end)
    long long slab_points;          // planes [p0, min(cubes_end, n0 - 1)] x n1 x n2
    int nblocks, contracted;
    float level;
    float origin[3], spacing[3], center[3];
    float radius;
};

__device__ __forceinline__ int axis_bit(int axis) { return 4 >> axis; }
// the k-th Kuhn tetrahedron: corner codes 0, bit(a), bit(a) | bit(b), 7 and the sign of the permutation (a, b, c)
__device__ __forceinline__ void kuhn(int k, int& c1, int& c2, int& sign)
{
    const int a = k >> 1, b = (a + 1 + (k & 1)) % 3;
    c1 = axis_bit(a); c2 = c1 | axis_bit(b);
    sign = (k & 1) ? -1 : 1;                                            // (a, a+1, a+2) is even, (a, a+2, a+1) odd
}

struct Corner { int i, j, k; long long g; };
__device__ __forceinline__ Corner slab_point(const MeshArgs& a, long long q)
{
    Corner c;
    c.k = (int)(q % a.n2);
    const long long r = q / a.n2;
    c.j = (int)(r % a.n1);
    c.i = a.p0 + (int)(r / a.n1);
    c.g = (long long)a.p0 * a.n1 * a.n2 + q;
    return c;
}
__device__ __forceinline__ long long code_offset(const MeshArgs& a, int c)
{
    return (long long)((c >> 2) & 1) * a.n1 * a.n2 + (long long)((c >> 1) & 1) * a.n2 + (c & 1);
}

__global__ __launch_bounds__(256) void mesh_count_kernel(MeshArgs a, const float* __restrict__ field, unsigned* __restrict__ words,
                                                         unsigned* __restrict__ block_count)
{
    __shared__ unsigned long long s_wave[4];
    const long long q = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
    unsigned mask = 0, ntri = 0, owned = 0;
    if (q < a.slab_points) {
        const Corner p = slab_point(a, q);
        const bool in0 = field[p.g] < a.level;
        unsigned in = in0 ? 1u : 0u;                                    // bit c: corner c of the cube is inside (missing corners: as corner 0)
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            const bool exists = p.i + ((c >> 2) & 1) < a.n0 && p.j + ((c >> 1) & 1) < a.n1 && p.k + (c & 1) < a.n2;
            const bool inc = exists ? field[p.g + code_offset(a, c)] < a.level : in0;
            in |= (inc ? 1u : 0u) << c;
            mask |= (inc != in0 ? 1u : 0u) << (c - 1);
        }
        if (p.i < a.cubes_end && p.i + 1 < a.n0 && p.j + 1 < a.n1 && p.k + 1 < a.n2) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                int c1, c2, sg;
                kuhn(t, c1, c2, sg);
                const unsigned ni = (in & 1u) + ((in >> c1) & 1u) + ((in >> c2) & 1u) + ((in >> 7) & 1u);
                ntri += (ni == 2u) ? 2u : (ni == 1u || ni == 3u) ? 1u : 0u;
            }
        }
        owned = p.i < a.own_end ? 1u : 0u;
    }
    const unsigned nv = __popc(mask);
    const unsigned long long c = pack_fields(nv, ntri, owned ? nv : 0u);
    unsigned long long total;
    const unsigned long long pre = block_exclusive_scan_256(c, s_wave, total);
    if (q < a.slab_points) words[q] = mask | (unpack_field(pre, 0) << 7) | (unpack_field(pre, 1) << 18);
    if (threadIdx.x < 3) block_count[(size_t)threadIdx.x * a.nblocks + blockIdx.x] = unpack_field(total, threadIdx.x);
}

// block_count [3][nblocks] (vertices, triangles, owned vertices); block_off [2][nblocks]; slab_base = run before this slab (0 for the
// first: nothing has to be cleared beforehand); run = slab_base + {owned, triangles}
__global__ __launch_bounds__(1024) void mesh_scan_kernel(int nblocks, const unsigned* __restrict__ block_count, unsigned* __restrict__ block_off,
                                                         long long* __restrict__ run, long long* __restrict__ slab_base, int first)
{
    __shared__ uint32_t s_wave[16];
    block_counts_exclusive_scan<1024>(nblocks, block_count, block_off, s_wave);
    const unsigned ntri = block_counts_exclusive_scan<1024>(nblocks, block_count + (size_t)nblocks, block_off + (size_t)nblocks, s_wave);
    const unsigned nown = block_counts_exclusive_scan<1024>(nblocks, block_count + 2 * (size_t)nblocks, nullptr, s_wave);
    if (threadIdx.x == 0) {
        const long long rv = first ? 0 : run[0], rt = first ? 0 : run[1];
        if (slab_base) { slab_base[0] = rv; slab_base[1] = rt; }
        run[0] = rv + (long long)nown;
        run[1] = rt + (long long)ntri;
    }
}

// index of the vertex on the edge from corner `lo` to corner `hi` (codes, lo a subset of hi) of the cube at slab point q
__device__ __forceinline__ int edge_vertex(const MeshArgs& a, const unsigned* __restrict__ words, const unsigned* __restrict__ block_off,
                                           long long vbase, long long q, int lo, int hi)
{
    const long long o = q + code_offset(a, lo);
    const unsigned w = words[o];
    const int dir = hi ^ lo;
    return (int)(vbase + block_off[o / MESH_BLOCK] + word_vpre(w) + __popc(word_mask(w) & ((1u << (dir - 1)) - 1u)));
}

__global__ __launch_bounds__(256) void mesh_emit_kernel(MeshArgs a, const float* __restrict__ field, const unsigned* __restrict__ words,
                                                        const unsigned* __restrict__ block_off, const long long* __restrict__ slab_base,
                                                        float* __restrict__ vertices, int* __restrict__ triangles)
{
    const long long q = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (q >= a.slab_points) return;
    const Corner p = slab_point(a, q);
    const unsigned w = words[q], mask = word_mask(w);
    const long long vbase = slab_base[0], tbase = slab_base[1];
    const float F0 = field[p.g];
    if (mask && p.i < a.own_end) {
        long long vi = vbase + block_off[blockIdx.x] + word_vpre(w);
        const float pa[3] = {a.origin[0] + a.spacing[0] * (float)p.i, a.origin[1] + a.spacing[1] * (float)p.j, a.origin[2] + a.spacing[2] * (float)p.k};
        const float pb[3] = {a.origin[0] + a.spacing[0] * (float)(p.i + 1), a.origin[1] + a.spacing[1] * (float)(p.j + 1),
                             a.origin[2] + a.spacing[2] * (float)(p.k + 1)};
#pragma unroll
        for (int c = 1; c < 8; ++c) {
            if (!((mask >> (c - 1)) & 1u)) continue;
            const float Fb = field[p.g + code_offset(a, c)];
            const float t = (a.level - F0) / (Fb - F0);
            float v[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) v[ax] = (c & axis_bit(ax)) ? pa[ax] + t * (pb[ax] - pa[ax]) : pa[ax];
            if (a.contracted) {                                         // mcube_utils.py:91-93
                const float mag = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                const float s = mag < 1.0f ? 1.0f : 1.0f / ((2.0f - mag) * mag);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) v[ax] = fminf(fmaxf(a.center[ax] + a.radius * (v[ax] * s), -32.0f), 32.0f);
            }
            vertices[3 * vi] = v[0]; vertices[3 * vi + 1] = v[1]; vertices[3 * vi + 2] = v[2];
            ++vi;
        }
    }
    if (!(p.i < a.cubes_end && p.i + 1 < a.n0 && p.j + 1 < a.n1 && p.k + 1 < a.n2)) return;
    unsigned in = F0 < a.level ? 1u : 0u;
#pragma unroll
    for (int c = 1; c < 8; ++c) in |= (((mask >> (c - 1)) ^ in) & 1u) << c;            // a crossing edge flips corner 0's side
    long long ti = tbase + block_off[(size_t)a.nblocks + blockIdx.x] + word_tpre(w);
    for (int t = 0; t < 6; ++t) {
        int c1, c2, sg;
        kuhn(t, c1, c2, sg);
        // corner code of vertex m of the tetrahedron: selects, not an indexed array (nothing here lives in scratch or LDS)
        auto code = [&](int m) { return m == 0 ? 0 : m == 1 ? c1 : m == 2 ? c2 : 7; };
        auto ev = [&](int m, int n) { return edge_vertex(a, words, block_off, vbase, q, code(m < n ? m : n), code(m < n ? n : m)); };
        const unsigned ins = (in & 1u) | (((in >> c1) & 1u) << 1) | (((in >> c2) & 1u) << 2) | (((in >> 7) & 1u) << 3);   // bit m: vertex m is inside
        const int ni = __popc(ins);
        if (ni == 0 || ni == 4) continue;
        int e0, e1, e2, f2 = 0;                                         // (e0, e1, e2) and, for two inside corners, (e0, e2, f2)
        bool flip;
        if (ni == 2) {
            // inside {ia, ib}, outside {oc, od}, each ascending: (ac, ad, bd) and (ac, bd, bc) wind as (ab, ac, ad) does for the tetrahedron
            // reordered (ia, ib, oc, od); that reordering is odd exactly when ib - ia == 2
            const unsigned outs = ~ins & 0xFu;
            const int ia = __ffs(ins) - 1, ib = 31 - __clz((int)ins), oc = __ffs(outs) - 1, od = 31 - __clz((int)outs);
            e0 = ev(ia, oc); e1 = ev(ia, od); e2 = ev(ib, od); f2 = ev(ib, oc);
            flip = (sg > 0) != (ib - ia != 2);
        } else {
            // the lone corner m against the other three in ascending order: moving it to the front takes m transpositions; a lone OUTSIDE
            // corner reverses the normal once more
            const unsigned lone = ni == 1 ? ins : (~ins & 0xFu);
            const int m = __ffs(lone) - 1;
            e0 = ev(m, m > 0 ? 0 : 1); e1 = ev(m, m > 1 ? 1 : 2); e2 = ev(m, m > 2 ? 2 : 3);
            flip = (((sg > 0) == ((m & 1) == 0)) == (ni == 1)) == false;
        }
        triangles[3 * ti] = e0; triangles[3 * ti + 1] = flip ? e2 : e1; triangles[3 * ti + 2] = flip ? e1 : e2;
        ++ti;
        if (ni == 2) {
            triangles[3 * ti] = e0; triangles[3 * ti + 1] = flip ? f2 : e2; triangles[3 * ti + 2] = flip ? e2 : f2;
            ++ti;
        }
    }
}

// ---- clusters --------------------------------------------------------------------------------------------------------------------
// cc_find / cc_union: mrgs_cc.h
__global__ __launch_bounds__(256) void cc_init_kernel(long long V, int* __restrict__ parent, int* __restrict__ counts)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V) { parent[v] = (int)v; counts[v] = 0; }
}
__global__ __launch_bounds__(256) void cc_hook_kernel(long long T, long long V, const int* __restrict__ tri, int* parent)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if ((unsigned)a >= (unsigned long long)V || (unsigned)b >= (unsigned long long)V || (unsigned)c >= (unsigned long long)V) return;
    cc_union(parent, a, b);
    cc_union(parent, a, c);
}
__global__ __launch_bounds__(256) void cc_flatten_kernel(long long V, int* parent)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V) {
        const int r = cc_find(parent, (int)v);                           // roots stay roots here: writing r over a link keeps every walk valid
        __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__global__ __launch_bounds__(256) void cc_count_kernel(long long T, long long V, const int* __restrict__ tri, const int* __restrict__ labels,
                                                       int* __restrict__ counts)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int a = tri[3 * t];
    if ((unsigned)a < (unsigned long long)V) atomicAdd(counts + labels[a], 1);
}
__global__ __launch_bounds__(256) void mesh_select_kernel(long long V, long long T, const int* __restrict__ tri, const int* __restrict__ labels,
                                                          const int* __restrict__ counts, int threshold, uint8_t* __restrict__ keep_v,
                                                          uint8_t* __restrict__ keep_t)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < V) keep_v[i] = counts[labels[i]] >= threshold ? 1 : 0;
    if (i < T) {
        const int a = tri[3 * i];
        keep_t[i] = ((unsigned)a < (unsigned long long)V && counts[labels[a]] >= threshold) ? 1 : 0;
    }
}
__global__ __launch_bounds__(256) void mesh_remap_kernel(long long V_new, long long V_old, const int* __restrict__ new_to_old, int* __restrict__ remap)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < V_new) { const int o = new_to_old[i]; if ((unsigned)o < (unsigned long long)V_old) remap[o] = (int)i; }
}
__global__ __launch_bounds__(256) void mesh_reindex_kernel(long long n, long long V_old, const int* __restrict__ remap, int* __restrict__ tri)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const int o = tri[i]; if ((unsigned)o < (unsigned long long)V_old) tri[i] = remap[o]; }
}

inline unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct MeshWs { unsigned* words; unsigned* counts; unsigned* offs; long long* run; long long* slab_base; size_t total; };

inline long long slab_points_max(const MrgsMeshConfig* cfg)
{
    const long long planes = (long long)(cfg->slab_planes < cfg->n0 - 1 ? cfg->slab_planes : cfg->n0 - 1) + 1;
    const long long plane = (long long)cfg->n1 * cfg->n2;
    return plane > MESH_MAX_SLAB_POINTS ? MESH_MAX_SLAB_POINTS + 1 : planes * plane;     // (no overflow: planes <= 2^31, plane <= 2^28)
}
MeshWs mesh_carve(void* base, long long points)
{
    const size_t nb = (size_t)((points + MESH_BLOCK - 1) / MESH_BLOCK);
    const size_t words = 0;
    const size_t counts = words + mrgs_align_up(nb * MESH_BLOCK * sizeof(unsigned), 256);
    const size_t offs = counts + mrgs_align_up(3 * nb * sizeof(unsigned), 256);
    const size_t run = offs + mrgs_align_up(2 * nb * sizeof(unsigned), 256);
    MeshWs w = {};
    w.total = run + 256;
    if (base) {                                                         // the size query carves nothing
        uint8_t* p = (uint8_t*)base;
        w.words = (unsigned*)(p + words); w.counts = (unsigned*)(p + counts); w.offs = (unsigned*)(p + offs);
        w.run = (long long*)(p + run); w.slab_base = w.run + 2;
    }
    return w;
}

int mesh_check_cfg(const MrgsMeshConfig* cfg)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsMeshConfig)) return MRGS_E_BAD_ARG;
    if (cfg->n0 < 2 || cfg->n1 < 2 || cfg->n2 < 2 || cfg->slab_planes < 1) return MRGS_E_BAD_ARG;
    for (int ax = 0; ax < 3; ++ax) if (!(cfg->spacing[ax] > 0.0f)) return MRGS_E_BAD_ARG;
    if (!(cfg->level == cfg->level)) return MRGS_E_BAD_ARG;
    if (cfg->contracted && !(cfg->radius > 0.0f)) return MRGS_E_BAD_ARG;
    if (slab_points_max(cfg) > MESH_MAX_SLAB_POINTS) return MRGS_E_UNSUPPORTED;
    return MRGS_OK;
}

// the count and scan launches of one slab; returns the slab's MeshArgs
MeshArgs mesh_slab(const MrgsMeshConfig* cfg, int p0, const float* field, const MeshWs& w, long long* run, long long* slab_base, hipStream_t st)
{
    MeshArgs a;
    a.n0 = cfg->n0; a.n1 = cfg->n1; a.n2 = cfg->n2;
    a.p0 = p0;
    a.cubes_end = p0 + cfg->slab_planes < cfg->n0 - 1 ? p0 + cfg->slab_planes : cfg->n0 - 1;
    a.own_end = a.cubes_end == cfg->n0 - 1 ? cfg->n0 : a.cubes_end;      // the last slab owns the last plane's in-plane edges too
    a.slab_points = (long long)(a.cubes_end - p0 + 1) * cfg->n1 * cfg->n2;
    a.nblocks = (int)((a.slab_points + MESH_BLOCK - 1) / MESH_BLOCK);
    a.contracted = cfg->contracted; a.level = cfg->level; a.radius = cfg->radius;
    for (int ax = 0; ax < 3; ++ax) { a.origin[ax] = cfg->origin[ax]; a.spacing[ax] = cfg->spacing[ax]; a.center[ax] = cfg->center[ax]; }
    mesh_count_kernel<<<dim3((unsigned)a.nblocks), 256, 0, st>>>(a, field, w.words, w.counts);
    mesh_scan_kernel<<<1, 1024, 0, st>>>(a.nblocks, w.counts, w.offs, run, slab_base, p0 == 0);
    return a;
}

}   // namespace

extern "C" int mrgs_tsdf_fuse(const MrgsTsdfConfig* cfg, const MrgsTsdfView* views, float* field, float* weight_debug, void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsTsdfConfig)) return MRGS_E_BAD_ARG;
    if (cfg->mode < MRGS_TSDF_CONTRACTED || cfg->mode > MRGS_TSDF_POINTS || cfg->n_views < 0 || !(cfg->trunc > 0.0f)) return MRGS_E_BAD_ARG;
    long long n;
    if (cfg->mode == MRGS_TSDF_POINTS) {
        if (cfg->n_points < 0) return MRGS_E_BAD_ARG;
        n = cfg->n_points;
    } else {
        if (cfg->n0 < 2 || cfg->n1 < 2 || cfg->n2 < 2) return MRGS_E_BAD_ARG;
        n = (long long)cfg->n0 * cfg->n1 * cfg->n2;
        if (cfg->mode == MRGS_TSDF_CONTRACTED && !(cfg->radius > 0.0f)) return MRGS_E_BAD_ARG;
    }
    if (n >= (1ll << 31) * 256) return MRGS_E_UNSUPPORTED;
    if (n == 0) return MRGS_OK;
    if (!field || (cfg->n_views > 0 && !views) || (cfg->mode == MRGS_TSDF_POINTS && !cfg->points)) return MRGS_E_BAD_ARG;
    FuseArgs a;
    a.mode = cfg->mode; a.n0 = cfg->n0; a.n1 = cfg->n1; a.n2 = cfg->n2; a.n_views = cfg->n_views; a.n = n;
    for (int ax = 0; ax < 3; ++ax) { a.origin[ax] = cfg->origin[ax]; a.spacing[ax] = cfg->spacing[ax]; a.center[ax] = cfg->center[ax]; }
    a.radius = cfg->radius; a.trunc = cfg->trunc; a.depth_trunc = cfg->depth_trunc; a.points = cfg->points;
    tsdf_fuse_kernel<<<dim3(blocks256(n)), 256, 0, (hipStream_t)stream>>>(a, views, field, weight_debug);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_vertex_fuse(const MrgsVertexFuseConfig* cfg, const MrgsAttrView* views, const float* points, float* out, float* weight,
                                void* stream)
{
    if (!cfg || cfg->struct_size != sizeof(MrgsVertexFuseConfig)) return MRGS_E_BAD_ARG;
    const int cp = cfg->channels;
    if ((cp != 4 && cp != 8 && cp != 12 && cp != 16) || (cfg->w0 != 0 && cfg->w0 != 1) || !(cfg->trunc > 0.0f)) return MRGS_E_BAD_ARG;
    if (cfg->n_views < 0 || cfg->n_points < 0) return MRGS_E_BAD_ARG;
    const long long n = cfg->n_points;
    if (n >= (1ll << 31) * 256) return MRGS_E_UNSUPPORTED;
    if (n == 0) return MRGS_OK;
    if (!points || !out || ((uintptr_t)out & 15) || (cfg->n_views > 0 && !views)) return MRGS_E_BAD_ARG;
    VertexFuseArgs a;
    a.n_views = cfg->n_views; a.n = n; a.w0 = (float)cfg->w0; a.trunc = cfg->trunc; a.depth_trunc = cfg->depth_trunc;
    const dim3 grid(blocks256(n));
    hipStream_t st = (hipStream_t)stream;
    switch (cp) {
    case 4: vertex_fuse_kernel<4><<<grid, 256, 0, st>>>(a, views, points, out, weight); break;
    case 8: vertex_fuse_kernel<8><<<grid, 256, 0, st>>>(a, views, points, out, weight); break;
    case 12: vertex_fuse_kernel<12><<<grid, 256, 0, st>>>(a, views, points, out, weight); break;
    default: vertex_fuse_kernel<16><<<grid, 256, 0, st>>>(a, views, points, out, weight); break;
    }
    return MRGS_LAUNCH_STATUS();
}

extern "C" size_t mrgs_mesh_ws_bytes(const MrgsMeshConfig* cfg)
{
    if (mesh_check_cfg(cfg) != MRGS_OK) return 0;
    return mesh_carve(nullptr, slab_points_max(cfg)).total;
}

extern "C" int mrgs_mesh_count(const MrgsMeshConfig* cfg, const float* field, void* ws, size_t ws_bytes, int64_t* totals_dev, void* stream)
{
    if (int rc = mesh_check_cfg(cfg)) return rc;
    if (!field || !ws || ((uintptr_t)ws & 7) || !totals_dev) return MRGS_E_BAD_ARG;
    if (ws_bytes < mrgs_mesh_ws_bytes(cfg)) return MRGS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const MeshWs w = mesh_carve(ws, slab_points_max(cfg));
    for (int p0 = 0; p0 < cfg->n0 - 1; p0 += cfg->slab_planes) mesh_slab(cfg, p0, field, w, (long long*)totals_dev, nullptr, st);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_mesh_emit(const MrgsMeshConfig* cfg, const float* field, void* ws, size_t ws_bytes, const int64_t* totals_host,
                              float* vertices, int32_t* triangles, void* stream)
{
    if (int rc = mesh_check_cfg(cfg)) return rc;
    if (!totals_host) return MRGS_E_BAD_ARG;
    const int64_t V = totals_host[0], T = totals_host[1];
    if (V < 0 || T < 0) return MRGS_E_BAD_ARG;
    if (V > 0x7FFFFFFFll || T > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
    if (V == 0 && T == 0) return MRGS_OK;                                // nothing to write: the destinations may be NULL
    if (!field || !ws || ((uintptr_t)ws & 7) || (V > 0 && !vertices) || (T > 0 && !triangles)) return MRGS_E_BAD_ARG;
    if (ws_bytes < mrgs_mesh_ws_bytes(cfg)) return MRGS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const MeshWs w = mesh_carve(ws, slab_points_max(cfg));
    for (int p0 = 0; p0 < cfg->n0 - 1; p0 += cfg->slab_planes) {
        const MeshArgs a = mesh_slab(cfg, p0, field, w, w.run, w.slab_base, st);
        mesh_emit_kernel<<<dim3((unsigned)a.nblocks), 256, 0, st>>>(a, field, w.words, w.offs, w.slab_base, vertices, triangles);
    }
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_mesh_clusters(int64_t V, int64_t T, const int32_t* triangles, int32_t* labels, int32_t* counts, void* stream)
{
    if (V < 0 || T < 0) return MRGS_E_BAD_ARG;
    if (V > 0x7FFFFFFFll || T > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
    if (V == 0) return MRGS_OK;
    if (!labels || !counts || (T > 0 && !triangles)) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    cc_init_kernel<<<dim3(blocks256(V)), 256, 0, st>>>(V, labels, counts);
    if (T > 0) cc_hook_kernel<<<dim3(blocks256(T)), 256, 0, st>>>(T, V, triangles, labels);
    cc_flatten_kernel<<<dim3(blocks256(V)), 256, 0, st>>>(V, labels);
    if (T > 0) cc_count_kernel<<<dim3(blocks256(T)), 256, 0, st>>>(T, V, triangles, labels, counts);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_mesh_select(int64_t V, int64_t T, const int32_t* triangles, const int32_t* labels, const int32_t* counts, int32_t threshold,
                                uint8_t* keep_vertex, uint8_t* keep_triangle, void* stream)
{
    if (V < 0 || T < 0) return MRGS_E_BAD_ARG;
    if (V > 0x7FFFFFFFll || T > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
    if (V == 0 && T == 0) return MRGS_OK;
    if (!labels || !counts || (V > 0 && !keep_vertex) || (T > 0 && (!triangles || !keep_triangle)) || (V == 0 && T > 0)) return MRGS_E_BAD_ARG;
    mesh_select_kernel<<<dim3(blocks256(V > T ? V : T)), 256, 0, (hipStream_t)stream>>>(V, T, triangles, labels, counts, threshold, keep_vertex,
                                                                                         keep_triangle);
    return MRGS_LAUNCH_STATUS();
}

extern "C" int mrgs_mesh_reindex(int64_t V_old, int64_t V_new, const int32_t* new_to_old, int32_t* remap_ws, int64_t T, int32_t* triangles,
                                 void* stream)
{
    if (V_old < 0 || V_new < 0 || T < 0 || V_new > V_old) return MRGS_E_BAD_ARG;
    if (V_old > 0x7FFFFFFFll || T > 0x7FFFFFFFll) return MRGS_E_UNSUPPORTED;
    if (T == 0 || V_new == 0) return MRGS_OK;
    if (!new_to_old || !remap_ws || !triangles) return MRGS_E_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    mesh_remap_kernel<<<dim3(blocks256(V_new)), 256, 0, st>>>(V_new, V_old, new_to_old, remap_ws);
    mesh_reindex_kernel<<<dim3(blocks256(3 * T)), 256, 0, st>>>(3 * T, V_old, remap_ws, triangles);
    return MRGS_LAUNCH_STATUS();
}
