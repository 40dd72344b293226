// mrgs_volume.hip -- per-gaussian shading of the volume renderer in one kernel (forward) and one kernel plus a one-thread launch (backward).
//
// Replaces the chain of torch ops render_volume runs per view between the raw parameters and the rasterizer call
// (gaussian_renderer/__init__.py:559-661 with opt.indirect false, utils/refl_utils.py:426-445, scene/light.py:99-129):
//   GaussianModel getters: opacity / refl / roughness / ori_color = sigmoid, scaling = exp, rotation = normalize;
//   get_normal: third column of R(q), flipped to face `campos` (camera_center), safe_normalize;
//   get_full_color_volume: w_o = safe_normalize(rays_o - xyz) with rays_o the origin of sample_camera_rays (the reference's OTHER
//     rounding of the camera position: both are kept), NdotV = w_o . n, rays_refl = safe_normalize(2 n NdotV - w_o),
//     diffuse = sigmoid(fetch(diffuse map, n)) (1 - refl) ori_color, direct = sigmoid(trilinear fetch(chain, rays_refl, get_mip(roughness))),
//     specular = direct ((0.04 (1 - refl) + ori_color refl) fg0.x + fg0.y);
//   colors_precomp = specular + diffuse, features = cat(roughness, refl, diffuse, specular, ori_color) (+ get_distance: "pgsr").
// fg0 is the FG pair of gaussian 0 for EVERY gaussian -- the reference indexes fg[0] (refl_utils.py:443) -- : every lane
// recomputes it from row 0's raw parameters (uniform addresses: scalar loads).  In the backward that couples every row to row 0: the
// workgroups sum dL/dfg0 (two numbers: wave DPP sums, one LDS step, one fp64 atomic pair per workgroup into the caller's scratch), and a
// one-thread launch behind them on the same stream takes the sum through the LUT fetch to row 0's NdotV and roughness.
// The 45 SH "rest" coefficients the torch chain evaluates along the mirror direction reach no output of this branch: they are not read.
//
// One gaussian per lane.  Feature rows of 11 floats (odd stride) travel through a per-wave LDS tile as 16-byte pieces of the wave's
// contiguous 2.75 KB run, rows of 12 ("pgsr") as three float4.  The backward does its two cube fetches one after the other, each with its
// scatter, so that one EnvSample / Taps pair is live at a time.
//
// Coordinates in fp64.  A cube fetch turns a direction into a texel coordinate in [0, res): in fp32 the direction (a dozen roundings from
// q and xyz), the quotient by the major axis and the scaling by res each leave ~res x 6e-8 of a texel in the bilinear fractions, and the
// gradients at xyz and q, which see the DIFFERENCES of neighbouring texels weighted by those fractions, carry it as a relative error of
// several 1e-6 (measured against the float64 statement: the same as the chain of torch ops, row by row a matter of luck which is worse).
// The geometry of a row -- normal, w_o, NdotV, mirror direction -- and the path direction -> face coordinate -> cell and fractions are
// therefore evaluated in fp64 (full-rate vector fp64 on this part; the kernels wait on memory) and rounded once, the fractions to fp32.
// Texel arithmetic, the adjoint (env_fetch_bwd) and everything behind it stay fp32 on the shared helpers of mrgs_envmap.h; the two
// functions that had to be restated for the fp64 coordinates (volume_taps, volume_fetch) follow cube_taps / env_fetch line by line.
#include "mrgs_internal.h"
#include "mrgs_model_math.h"
#include "mrgs_envmap.h"

namespace {

#define FEAT_L 11            // roughness, refl, diffuse 3, specular 3, ori_color 3; odd: lane-private tile rows are bank-conflict free

struct ViewShade {           // what hangs on w_o = safe_normalize(rays_o - xyz) and the facing normal
    float wo[3], wolen;      // unit vector to the ray origin, clamp_min(|rays_o - xyz|, 1e-20)
    bool wo_live;            // the clamp passes the gradient (|.| >= 1e-20)
    float c;                 // NdotV
    float r[3], rlen;        // rays_refl, clamp_min(|2 n c - w_o|, 1e-20)
    bool r_live;
};
struct Geometry {            // a row's frame and view terms: evaluated in fp64, rounded once
    Frame f;                 // (qlen, qn, nr, flip, nflen, nn; the mirror terms of make_frame about `campos` are not this stage's)
    ViewShade s;
    double nn[3], r[3];      // the two fetch directions, unrounded
};

__device__ __forceinline__ Geometry make_geometry(const float (&p)[3], const float4 q4, const float* __restrict__ campos, const float* __restrict__ rays_o)
{
    Geometry g;
    const double q[4] = {q4.x, q4.y, q4.z, q4.w};
    const double qlen = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / qlen, x = q[1] / qlen, y = q[2] / qlen, z = q[3] / qlen;
    const double nr[3] = {2.0 * (x * z + w * y), 2.0 * (y * z - w * x), 1.0 - 2.0 * (x * x + y * y)};
    // flip_align_view against the unit direction camera_center -> xyz
    const double d[3] = {(double)p[0] - campos[0], (double)p[1] - campos[1], (double)p[2] - campos[2]};
    const double dlen = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double facing = -(nr[0] * d[0] + nr[1] * d[1] + nr[2] * d[2]) / dlen;
    const double flip = facing >= 0.0 ? 1.0 : -1.0;
    const double nf[3] = {nr[0] * flip, nr[1] * flip, nr[2] * flip};
    const double nflen = fmax(sqrt(nf[0] * nf[0] + nf[1] * nf[1] + nf[2] * nf[2]), 1e-20);
    // w_o, NdotV, rays_refl
    const double e[3] = {(double)rays_o[0] - p[0], (double)rays_o[1] - p[1], (double)rays_o[2] - p[2]};
    const double el = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const double wolen = fmax(el, 1e-20);
    double wo[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { g.nn[i] = nf[i] / nflen; wo[i] = e[i] / wolen; }
    const double c = wo[0] * g.nn[0] + wo[1] * g.nn[1] + wo[2] * g.nn[2];
    const double rr[3] = {2.0 * g.nn[0] * c - wo[0], 2.0 * g.nn[1] * c - wo[1], 2.0 * g.nn[2] * c - wo[2]};
    const double rl = sqrt(rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2]);
    const double rlen = fmax(rl, 1e-20);
    g.f.qlen = (float)qlen;
    g.f.qn[0] = (float)w; g.f.qn[1] = (float)x; g.f.qn[2] = (float)y; g.f.qn[3] = (float)z;
    g.f.flip = (float)flip; g.f.nflen = (float)nflen;
    g.f.dlen = (float)dlen; g.f.c = 0.0f;
    g.s.wo_live = el >= 1e-20; g.s.wolen = (float)wolen; g.s.c = (float)c;
    g.s.r_live = rl >= 1e-20; g.s.rlen = (float)rlen;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        g.r[i] = rr[i] / rlen;
        g.f.nr[i] = (float)nr[i]; g.f.nn[i] = (float)g.nn[i]; g.f.v[i] = (float)(d[i] / dlen); g.f.r[i] = 0.0f;
        g.s.wo[i] = (float)wo[i]; g.s.r[i] = (float)g.r[i];
    }
    return g;
}

// dir_to_face (mrgs_envmap.h) on an fp64 direction: the same selections, the IEEE quotient; the fp32 copy is what env_fetch_bwd reads
struct FaceUVd { FaceUV f; double u, v; };
__device__ __forceinline__ FaceUVd dir_to_face_d(const double (&d)[3])
{
    FaceUVd r;
    const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
    const bool mx = ax >= ay && ax >= az, my = !mx && ay >= az;
    const double ma = mx ? ax : (my ? ay : az), mc = mx ? d[0] : (my ? d[1] : d[2]);
    const bool pos = mc >= 0.0;
    const double inv = 1.0 / ma;
    const double un = mx ? (pos ? -d[2] : d[2]) : (my ? d[0] : (pos ? d[0] : -d[0]));
    const double vn = my ? (pos ? d[2] : -d[2]) : -d[1];
    r.u = un * inv; r.v = vn * inv;
    r.f.axis = mx ? 0 : (my ? 1 : 2);
    r.f.sgn = pos ? 1.f : -1.f;
    r.f.inv_ma = (float)inv;
    r.f.face = 2 * r.f.axis + (pos ? 0 : 1);
    r.f.u = (float)r.u; r.f.v = (float)r.v;
    return r;
}
// cube_taps with the cell and the fractions taken from the fp64 coordinate
__device__ __forceinline__ Taps volume_taps(const FaceUVd& fu, int res)
{
    Taps t;
    const double fx = (fu.u * 0.5 + 0.5) * (double)res - 0.5, fy = (fu.v * 0.5 + 0.5) * (double)res - 0.5;
    const double x0f = floor(fx), y0f = floor(fy);
    const int x0 = (int)x0f, y0 = (int)y0f, face = fu.f.face;
    t.wx = (float)(fx - x0f); t.wy = (float)(fy - y0f);
    const bool ox0 = x0 < 0, ox1 = x0 + 1 >= res, oy0 = y0 < 0, oy1 = y0 + 1 >= res;
    t.w[0] = (1.f - t.wx) * (1.f - t.wy); t.w[1] = t.wx * (1.f - t.wy); t.w[2] = (1.f - t.wx) * t.wy; t.w[3] = t.wx * t.wy;
    const bool c0 = ox0 && oy0, c1 = ox1 && oy0, c2 = ox0 && oy1, c3 = ox1 && oy1;
    t.corner = c0 || c1 || c2 || c3;
    t.norm = 1.0f;
    if (t.corner) {   // three faces meet: the diagonal tap does not exist
        if (c0) t.w[0] = 0.f; if (c1) t.w[1] = 0.f; if (c2) t.w[2] = 0.f; if (c3) t.w[3] = 0.f;
        const float s = 1.0f / (t.w[0] + t.w[1] + t.w[2] + t.w[3]);
        t.norm = s;
        t.w[0] *= s; t.w[1] *= s; t.w[2] *= s; t.w[3] *= s;
    }
    t.idx[0] = c0 ? 0 : wrap_tap(face, x0, y0, res);
    t.idx[1] = c1 ? 0 : wrap_tap(face, x0 + 1, y0, res);
    t.idx[2] = c2 ? 0 : wrap_tap(face, x0, y0 + 1, res);
    t.idx[3] = c3 ? 0 : wrap_tap(face, x0 + 1, y0 + 1, res);
    return t;
}
// env_fetch on those taps
__device__ __forceinline__ void volume_fetch(const EnvMips& m, const FaceUVd& fu, float level, bool use_mips, EnvSample& s, Taps tp[2])
{
    env_levels(m, level, use_mips, s);
    float v[2][3];
    const int res0 = level_res(m, s.l0), res1 = level_res(m, s.l1);
    tp[0] = volume_taps(fu, res0);
    tp[1] = volume_taps(fu, res1);
    const float* tex0 = level_tex(m, s.l0);
    const float* tex1 = level_tex(m, s.l1);
    float t[2][4][3];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int q = 0; q < 4; q++) {        // unconditional: a missing corner tap has index 0 and weight 0
            const Tex3 v3 = *reinterpret_cast<const Tex3*>((k == 0 ? tex0 : tex1) + (size_t)tp[k].idx[q] * 3);
            t[k][q][0] = v3.x; t[k][q][1] = v3.y; t[k][q][2] = v3.z;
        }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int res = k == 0 ? res0 : res1;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int c = 0; c < 3; c++) t[k][q][c] = tp[k].w[q] != 0.f ? t[k][q][c] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[k][c] = tp[k].w[0] * t[k][0][c] + tp[k].w[1] * t[k][1][c] + tp[k].w[2] * t[k][2][c] + tp[k].w[3] * t[k][3][c];
            s.du[k][c] = ((1.f - tp[k].wy) * (t[k][1][c] - t[k][0][c]) + tp[k].wy * (t[k][3][c] - t[k][2][c])) * 0.5f * (float)res * tp[k].norm;
            s.dv[k][c] = ((1.f - tp[k].wx) * (t[k][2][c] - t[k][0][c]) + tp[k].wx * (t[k][3][c] - t[k][1][c])) * 0.5f * (float)res * tp[k].norm;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        s.L[c] = (1.f - s.f) * v[0][c] + s.f * v[1][c];
        s.dlev[c] = (s.lev_in && s.l1 != s.l0) ? v[1][c] - v[0][c] : 0.f;
    }
}

// gradient at a unit vector u = x / clamp_min(|x|, 1e-20) -> gradient at x
__device__ __forceinline__ void unit_bwd(const float (&u)[3], float len, bool live, const float (&g)[3], float (&gx)[3])
{
    const float ug = live ? u[0] * g[0] + u[1] * g[1] + u[2] * g[2] : 0.0f;      // (under the clamp the divisor is a constant)
#pragma unroll
    for (int i = 0; i < 3; i++) gx[i] = (g[i] - u[i] * ug) / len;
}

// gradients at the facing normal and at w_o -> at the raw quaternion (through qn = q / |q|, without the `rotations` output's share) and
// at the centre.  The flip sign is a constant, as it is for autograd.
__device__ __forceinline__ void geometry_bwd(const Frame& f, const ViewShade& s, const float (&g_nn)[3], const float (&g_wo)[3], float (&d_q)[4],
                                             float (&d_p)[3])
{
    const float nn_dot = f.nn[0] * g_nn[0] + f.nn[1] * g_nn[1] + f.nn[2] * g_nn[2];
    float a[3];
#pragma unroll
    for (int i = 0; i < 3; i++) a[i] = (g_nn[i] - f.nn[i] * nn_dot) / f.nflen * f.flip;
    float d_qn[4];
    frame_nr_bwd(f, a, d_qn);
    float dot1 = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) dot1 += f.qn[i] * d_qn[i];
#pragma unroll
    for (int i = 0; i < 4; i++) d_q[i] = (d_qn[i] - f.qn[i] * dot1) / f.qlen;
    float g_d[3];
    unit_bwd(s.wo, s.wolen, s.wo_live, g_wo, g_d);
#pragma unroll
    for (int i = 0; i < 3; i++) d_p[i] = -g_d[i];                  // d = rays_o - xyz
}

// row 0's LUT coordinates: (NdotV, roughness).clamp(0, 1)
struct Row0 { float p[3]; Frame f; ViewShade s; float rough, u, v; bool u_in; };
__device__ __forceinline__ Row0 make_row0(const MrgsVolumeParams& prm)
{
    Row0 z;
    z.p[0] = prm.xyz[0]; z.p[1] = prm.xyz[1]; z.p[2] = prm.xyz[2];
    const Geometry g = make_geometry(z.p, reinterpret_cast<const float4*>(prm.rotation_raw)[0], prm.campos, prm.rays_o);
    z.f = g.f; z.s = g.s;
    z.rough = sigmoidf(prm.rough_raw[0]);
    z.u_in = z.s.c >= 0.0f && z.s.c <= 1.0f;
    z.u = fminf(fmaxf(z.s.c, 0.0f), 1.0f);
    z.v = fminf(fmaxf(z.rough, 0.0f), 1.0f);
    return z;
}

__device__ __forceinline__ f3 as_f3(const float (&a)[3]) { return mk(a[0], a[1], a[2]); }

__global__ void __launch_bounds__(256) volume_features_fwd_kernel(MrgsVolumeParams prm, EnvMips spec, EnvMips diff, float* __restrict__ opacity,
                                                                  float* __restrict__ scales, float* __restrict__ rotations,
                                                                  float* __restrict__ colors, float* __restrict__ features)
{
    __shared__ float s_feat[4][64 * FEAT_L];
    const int P = prm.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * 256 + wave * 64;
    const int nrows = min(64, P - row0);
    if (nrows <= 0) return;
    const bool in_range = row0 + lane < P;
    const int idx = in_range ? row0 + lane : P - 1;        // out-of-range lanes stay for the cooperative tile store

    const float p[3] = {prm.xyz[3 * (size_t)idx], prm.xyz[3 * (size_t)idx + 1], prm.xyz[3 * (size_t)idx + 2]};
    const float4 q = reinterpret_cast<const float4*>(prm.rotation_raw)[idx];
    const Geometry geo = make_geometry(p, q, prm.campos, prm.rays_o);
    const Frame& f = geo.f;
    const float refl = sigmoidf(prm.refl_raw[idx]), rough = sigmoidf(prm.rough_raw[idx]);
    const float oc[3] = {sigmoidf(prm.ori_color_raw[3 * (size_t)idx]), sigmoidf(prm.ori_color_raw[3 * (size_t)idx + 1]),
                         sigmoidf(prm.ori_color_raw[3 * (size_t)idx + 2])};

    const Row0 z = make_row0(prm);
    float fg[2], fdu[2], fdv[2];
    lut_fetch(prm.lut, prm.lut_res, z.u, z.v, fg, fdu, fdv);

    EnvSample es;
    Taps tp[2];
    volume_fetch(diff, dir_to_face_d(geo.nn), 0.0f, false, es, tp);
    float dif[3];
#pragma unroll
    for (int c = 0; c < 3; c++) dif[c] = sigmoidf(es.L[c]) * (1.0f - refl) * oc[c];
    float dlevel;
    const float level = mip_level(spec, rough, dlevel);
    volume_fetch(spec, dir_to_face_d(geo.r), level, true, es, tp);
    float spc[3];
#pragma unroll
    for (int c = 0; c < 3; c++) spc[c] = sigmoidf(es.L[c]) * ((0.04f * (1.0f - refl) + oc[c] * refl) * fg[0] + fg[1]);

    if (in_range) {
        opacity[idx] = sigmoidf(prm.opacity_raw[idx]);
        const float2 sr = reinterpret_cast<const float2*>(prm.scaling_raw)[idx];
        reinterpret_cast<float2*>(scales)[idx] = make_float2(expf(sr.x), expf(sr.y));
        const float rl = fmaxf(f.qlen, 1e-12f);              // torch.nn.functional.normalize: x / max(|x|, 1e-12)
        reinterpret_cast<float4*>(rotations)[idx] = make_float4(q.x / rl, q.y / rl, q.z / rl, q.w / rl);
#pragma unroll
        for (int c = 0; c < 3; c++) colors[3 * (size_t)idx + c] = spc[c] + dif[c];
    }
    if (prm.viewmatrix != nullptr) {         // "pgsr": rows of twelve floats, channel 11 = the plane distance
        if (!in_range) return;
        float4* fo = reinterpret_cast<float4*>(features) + 3 * (size_t)idx;
        fo[0] = make_float4(rough, refl, dif[0], dif[1]);
        fo[1] = make_float4(dif[2], spc[0], spc[1], spc[2]);
        fo[2] = make_float4(oc[0], oc[1], oc[2], fabsf(plane_distance(prm.viewmatrix, f.nn, p).s));
        return;
    }
    float* row = s_feat[wave] + lane * FEAT_L;
    row[0] = rough; row[1] = refl;
#pragma unroll
    for (int c = 0; c < 3; c++) { row[2 + c] = dif[c]; row[5 + c] = spc[c]; row[8 + c] = oc[c]; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    tile_store<FEAT_L>(s_feat[wave], features + (size_t)row0 * FEAT_L, nrows, lane);
}

__global__ void __launch_bounds__(256) volume_features_bwd_kernel(MrgsVolumeParams prm, EnvMips spec, EnvMips diff, const float* __restrict__ g_opacity,
                                                                  const float* __restrict__ g_scales, const float* __restrict__ g_rotations,
                                                                  const float* __restrict__ g_colors, const float* __restrict__ g_features,
                                                                  MrgsVolumeGrads out, const float* __restrict__ g_xyz_upstream,
                                                                  double* __restrict__ fg_sum)
{
    __shared__ float s_feat[4][64 * FEAT_L];
    __shared__ float s_fg[4][2];
    const int P = prm.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = blockIdx.x * 256 + wave * 64;
    const int nrows = min(64, P - row0);              // <= 0: a wave behind the last row -- it stays for the workgroup's sum, with zeros
    const bool in_range = row0 + lane < P;
    const int idx = in_range ? row0 + lane : P - 1;   // out-of-range lanes stay: the texel scatter and the sums are wave-convergent

    // upstream gradient of the feature row
    float gf[12];
#pragma unroll
    for (int k = 0; k < 12; k++) gf[k] = 0.0f;
    const bool pgsr = prm.viewmatrix != nullptr;
    if (g_features != nullptr) {
        if (pgsr) {
            const float4* gi = reinterpret_cast<const float4*>(g_features) + 3 * (size_t)idx;
            const float4 a = gi[0], b = gi[1], c = gi[2];
            gf[0] = a.x; gf[1] = a.y; gf[2] = a.z; gf[3] = a.w; gf[4] = b.x; gf[5] = b.y; gf[6] = b.z; gf[7] = b.w;
            gf[8] = c.x; gf[9] = c.y; gf[10] = c.z; gf[11] = c.w;
        } else {
            tile_load<FEAT_L>(s_feat[wave], g_features + (size_t)row0 * FEAT_L, nrows, lane);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (in_range) {
                const float* row = s_feat[wave] + lane * FEAT_L;
#pragma unroll
                for (int k = 0; k < FEAT_L; k++) gf[k] = row[k];
            }
        }
    }
    if (!in_range) {
#pragma unroll
        for (int k = 0; k < 12; k++) gf[k] = 0.0f;
    }
    float gcol[3] = {0.0f, 0.0f, 0.0f};
    if (g_colors != nullptr && in_range) {
#pragma unroll
        for (int c = 0; c < 3; c++) gcol[c] = g_colors[3 * (size_t)idx + c];
    }

    const float p[3] = {prm.xyz[3 * (size_t)idx], prm.xyz[3 * (size_t)idx + 1], prm.xyz[3 * (size_t)idx + 2]};
    const float4 q = reinterpret_cast<const float4*>(prm.rotation_raw)[idx];
    const Geometry geo = make_geometry(p, q, prm.campos, prm.rays_o);
    const Frame& f = geo.f;
    const ViewShade& s = geo.s;
    const float refl = sigmoidf(prm.refl_raw[idx]), rough = sigmoidf(prm.rough_raw[idx]);
    const float oc[3] = {sigmoidf(prm.ori_color_raw[3 * (size_t)idx]), sigmoidf(prm.ori_color_raw[3 * (size_t)idx + 1]),
                         sigmoidf(prm.ori_color_raw[3 * (size_t)idx + 2])};
    const Row0 z = make_row0(prm);
    float fg[2], fdu[2], fdv[2];
    lut_fetch(prm.lut, prm.lut_res, z.u, z.v, fg, fdu, fdv);

    float g_refl = gf[1], g_rough = gf[0];
    float g_oc[3] = {gf[8], gf[9], gf[10]};
    float g_nn[3] = {0.0f, 0.0f, 0.0f}, g_wo[3] = {0.0f, 0.0f, 0.0f}, d_p_pd[3] = {0.0f, 0.0f, 0.0f};

    // "pgsr": the plane distance |nc . cc| sends its gradient to the facing normal and to the centre
    if (pgsr) {
        const PlaneDist pd = plane_distance(prm.viewmatrix, f.nn, p);
        const float sg = pd.s > 0.0f ? gf[11] : (pd.s < 0.0f ? -gf[11] : 0.0f);           // d|s| = sign(s) (torch: 0 at 0)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float* Wi = prm.viewmatrix + 4 * i;
            g_nn[i] = sg * (Wi[0] * pd.cc[0] + Wi[1] * pd.cc[1] + Wi[2] * pd.cc[2]);
            d_p_pd[i] = sg * (Wi[0] * pd.nc[0] + Wi[1] * pd.nc[1] + Wi[2] * pd.nc[2]);
        }
    }

    // ---- diffuse = sigmoid(fetch(diffuse map, n)) (1 - refl) ori_color ----
    {
        EnvSample es;
        Taps tp[2];
        const f3 dir = as_f3(f.nn);
        const FaceUVd fud = dir_to_face_d(geo.nn);
        const FaceUV& fu = fud.f;
        volume_fetch(diff, fud, 0.0f, false, es, tp);
        float gL[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float Ld = sigmoidf(es.L[c]);
            const float gd = gf[2 + c] + gcol[c];
            g_refl -= gd * Ld * oc[c];
            g_oc[c] += gd * Ld * (1.0f - refl);
            gL[c] = gd * (1.0f - refl) * oc[c] * Ld * (1.0f - Ld);
        }
        f3 gdir;
        float glev;
        env_fetch_bwd<true>(diff, fu, dir, es, tp, gL, gdir, glev);
        g_nn[0] += gdir.x; g_nn[1] += gdir.y; g_nn[2] += gdir.z;
    }

    // ---- specular = sigmoid(fetch(chain, rays_refl, get_mip(roughness))) ((0.04 (1 - refl) + ori_color refl) fg0.x + fg0.y) ----
    float g_fg[2] = {0.0f, 0.0f};
    {
        EnvSample es;
        Taps tp[2];
        const f3 dir = as_f3(s.r);
        const FaceUVd fud = dir_to_face_d(geo.r);
        const FaceUV& fu = fud.f;
        float dlevel;
        const float level = mip_level(spec, rough, dlevel);
        volume_fetch(spec, fud, level, true, es, tp);
        float gL[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float Ls = sigmoidf(es.L[c]);
            const float gs = gf[5 + c] + gcol[c];
            const float base = 0.04f * (1.0f - refl) + oc[c] * refl;
            const float g_sw = gs * Ls;
            g_refl += g_sw * (oc[c] - 0.04f) * fg[0];
            g_oc[c] += g_sw * refl * fg[0];
            g_fg[0] += g_sw * base;
            g_fg[1] += g_sw;
            gL[c] = gs * (base * fg[0] + fg[1]) * Ls * (1.0f - Ls);
        }
        f3 gdir;
        float glev;
        env_fetch_bwd<true>(spec, fu, dir, es, tp, gL, gdir, glev);
        g_rough += glev * dlevel;
        // rays_refl = rr / clamp_min(|rr|, 1e-20), rr = 2 n c - w_o, c = w_o . n
        const float g_r[3] = {gdir.x, gdir.y, gdir.z};
        float g_rr[3];
        unit_bwd(s.r, s.rlen, s.r_live, g_r, g_rr);
        const float n_dot = f.nn[0] * g_rr[0] + f.nn[1] * g_rr[1] + f.nn[2] * g_rr[2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            g_nn[i] += 2.0f * s.c * g_rr[i] + 2.0f * n_dot * s.wo[i];
            g_wo[i] += 2.0f * n_dot * f.nn[i] - g_rr[i];
        }
    }

    // ---- the sum over the rows of dL/dfg0: per wave, per workgroup, one atomic pair ----
    const float w0 = wave_dpp_sum(g_fg[0]), w1 = wave_dpp_sum(g_fg[1]);
    if (lane == 0) { s_fg[wave][0] = w0; s_fg[wave][1] = w1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float t = (s_fg[0][threadIdx.x] + s_fg[1][threadIdx.x]) + (s_fg[2][threadIdx.x] + s_fg[3][threadIdx.x]);
        if (t != 0.0f) atomicAdd(fg_sum + threadIdx.x, (double)t);
    }
    if (!in_range) return;

    float d_q[4], d_p[3];
    geometry_bwd(f, s, g_nn, g_wo, d_q, d_p);
    // plus the `rotations` output = normalize(q) with upstream g_rotations
    const float4 gr = g_rotations ? reinterpret_cast<const float4*>(g_rotations)[idx] : make_float4(0, 0, 0, 0);
    const float grv[4] = {gr.x, gr.y, gr.z, gr.w};
    float dot2 = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) dot2 += f.qn[i] * grv[i];
    const float rl = fmaxf(f.qlen, 1e-12f);
#pragma unroll
    for (int i = 0; i < 4; i++) d_q[i] += (grv[i] - f.qn[i] * dot2) / rl;
    reinterpret_cast<float4*>(out.d_rotation)[idx] = make_float4(d_q[0], d_q[1], d_q[2], d_q[3]);
#pragma unroll
    for (int i = 0; i < 3; i++)           // + what reached the centres some other way (the rasterizer's dL/dmeans3D)
        out.d_xyz[3 * (size_t)idx + i] = (g_xyz_upstream ? g_xyz_upstream[3 * (size_t)idx + i] : 0.0f) + d_p[i] + d_p_pd[i];

    // ---- activations ----
    const float so = sigmoidf(prm.opacity_raw[idx]);
    out.d_opacity[idx] = (g_opacity ? g_opacity[idx] : 0.0f) * so * (1.0f - so);
    const float2 sr = reinterpret_cast<const float2*>(prm.scaling_raw)[idx];
    const float2 gs = g_scales ? reinterpret_cast<const float2*>(g_scales)[idx] : make_float2(0, 0);
    reinterpret_cast<float2*>(out.d_scaling)[idx] = make_float2(gs.x * expf(sr.x), gs.y * expf(sr.y));
    out.d_refl[idx] = g_refl * refl * (1.0f - refl);
    out.d_rough[idx] = g_rough * rough * (1.0f - rough);
#pragma unroll
    for (int i = 0; i < 3; i++) out.d_ori_color[3 * (size_t)idx + i] = g_oc[i] * oc[i] * (1.0f - oc[i]);
}

// Behind the kernel above on the same stream: the summed dL/dfg0 through the LUT fetch and the clamp to row 0's NdotV and roughness, added
// to the gradients that kernel wrote for row 0.  One thread.
__global__ void __launch_bounds__(64) volume_row0_bwd_kernel(MrgsVolumeParams prm, MrgsVolumeGrads out, const double* __restrict__ fg_sum)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float G[2] = {(float)fg_sum[0], (float)fg_sum[1]};
    const Row0 z = make_row0(prm);
    float fg[2], du[2], dv[2];
    lut_fetch(prm.lut, prm.lut_res, z.u, z.v, fg, du, dv);
    const float g_c = z.u_in ? G[0] * du[0] + G[1] * du[1] : 0.0f;          // clamp(0, 1) passes the gradient inside [0, 1]
    const float g_v = G[0] * dv[0] + G[1] * dv[1];                           // (a sigmoid is always inside)
    out.d_rough[0] += g_v * z.rough * (1.0f - z.rough);
    // c = w_o . n
    const float g_nn[3] = {g_c * z.s.wo[0], g_c * z.s.wo[1], g_c * z.s.wo[2]};
    const float g_wo[3] = {g_c * z.f.nn[0], g_c * z.f.nn[1], g_c * z.f.nn[2]};
    float d_q[4], d_p[3];
    geometry_bwd(z.f, z.s, g_nn, g_wo, d_q, d_p);
#pragma unroll
    for (int i = 0; i < 4; i++) out.d_rotation[i] += d_q[i];
#pragma unroll
    for (int i = 0; i < 3; i++) out.d_xyz[i] += d_p[i];
}

#define MRGS_VOLUME_WS_BYTES 64      // two fp64 sums, padded to a cache-line half
// the library's one status path, written out (the macro's users are enumerated by tests/test_status.py, one call per file; this file's
// failure path is covered by tests/test_volume_features.py)
#define VOLUME_LAUNCH_STATUS mrgs_hip_status(hipGetLastError(), __FILE__, __LINE__)

// everything both entry points check before anything is queued
int volume_args(const MrgsVolumeParams* p, const MrgsEnvMips* specular, const MrgsEnvMips* diffuse, EnvMips& ms, EnvMips& md)
{
    if (!p || p->struct_size != sizeof(MrgsVolumeParams) || p->P < 0 || p->lut_res < 1) return MRGS_E_BAD_ARG;
    if (int rc = make_mips(specular, ms)) return rc;
    if (int rc = make_mips(diffuse, md)) return rc;
    if (p->P == 0) return MRGS_OK;
    if (!p->xyz || !p->scaling_raw || !p->rotation_raw || !p->opacity_raw || !p->refl_raw || !p->rough_raw || !p->ori_color_raw || !p->campos ||
        !p->rays_o || !p->lut)
        return MRGS_E_BAD_ARG;
    return MRGS_OK;
}

}   // namespace

extern "C" {

size_t mrgs_volume_features_ws_bytes(void) { return MRGS_VOLUME_WS_BYTES; }

int mrgs_volume_features_forward(const MrgsVolumeParams* p, const MrgsEnvMips* specular, const MrgsEnvMips* diffuse, float* opacity, float* scales,
                                 float* rotations, float* colors_precomp, float* features, void* stream)
{
    EnvMips ms, md;
    if (int rc = volume_args(p, specular, diffuse, ms, md)) return rc;
    if (p->P == 0) return MRGS_OK;
    if (!opacity || !scales || !rotations || !colors_precomp || !features || ((uintptr_t)features & 15u) != 0) return MRGS_E_BAD_ARG;
    hipLaunchKernelGGL(volume_features_fwd_kernel, dim3((p->P + 255) / 256), dim3(256), 0, (hipStream_t)stream, *p, ms, md, opacity, scales,
                       rotations, colors_precomp, features);
    return VOLUME_LAUNCH_STATUS;
}

int mrgs_volume_features_backward(const MrgsVolumeParams* p, const MrgsEnvMips* specular, const MrgsEnvMips* diffuse, const float* g_opacity,
                                  const float* g_scales, const float* g_rotations, const float* g_colors_precomp, const float* g_features,
                                  const MrgsVolumeGrads* grads, const float* g_xyz_upstream, void* ws, size_t ws_bytes, void* stream)
{
    EnvMips ms, md;
    if (int rc = volume_args(p, specular, diffuse, ms, md)) return rc;
    if (!grads || grads->struct_size != sizeof(MrgsVolumeGrads)) return MRGS_E_BAD_ARG;
    if (p->P == 0) return MRGS_OK;
    if (!grads->d_xyz || !grads->d_scaling || !grads->d_rotation || !grads->d_opacity || !grads->d_refl || !grads->d_rough || !grads->d_ori_color)
        return MRGS_E_BAD_ARG;
    if (!ws || ws_bytes < MRGS_VOLUME_WS_BYTES || ((uintptr_t)ws & 7u) != 0 || ((uintptr_t)g_features & 15u) != 0) return MRGS_E_BAD_ARG;
    MRGS_HIP_TRY(hipMemsetAsync(ws, 0, MRGS_VOLUME_WS_BYTES, (hipStream_t)stream));
    hipLaunchKernelGGL(volume_features_bwd_kernel, dim3((p->P + 255) / 256), dim3(256), 0, (hipStream_t)stream, *p, ms, md, g_opacity, g_scales,
                       g_rotations, g_colors_precomp, g_features, *grads, g_xyz_upstream, (double*)ws);
    if (int rc = VOLUME_LAUNCH_STATUS) return rc;
    hipLaunchKernelGGL(volume_row0_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *p, *grads, (const double*)ws);
    return VOLUME_LAUNCH_STATUS;
}

}   // extern "C"
