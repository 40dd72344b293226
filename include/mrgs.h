/*
 * mrgs.h -- C ABI of libmrgs.so, the MI355X (gfx950) surfel rasterizer + BRDF shading library.
 *
 * Drop-in boundary for the reference's rasterizer extension `diff_surfel_rasterization._C`
 * (pybind: /root/reference/submodules/diff-surfel-rasterization/ext.cpp:15-19).  Every entry point below
 * names the reference interface it replaces.  Plain pointers and sizes only -- no torch types; every
 * pointer is a DEVICE pointer unless its name ends in _host.  The library never allocates or frees device
 * memory: the caller owns the outputs and the three opaque workspaces (sizes from mrgs_*_bytes), exactly as
 * the reference's geomBuffer / binningBuffer / imgBuffer tensors are owned by Python
 * (rasterize_points.cu:95-103, diff_surfel_rasterization/__init__.py:101).  ONE exception, host memory: the forward calls that
 * report the pair count without a blocking copy (mrgs_rasterize_forward, _begin / _finish) read it from a pinned, device-mapped
 * slot; the library allocates a ring of MRGS_TICKET_RING (16) such 64-byte slots per (host thread, device) with hipHostMalloc on
 * first use and keeps it for the life of the process.  Consequence: a ticket of mrgs_rasterize_forward_begin is finished on the
 * SAME host thread that began it (the ring is thread-local; another thread's _finish returns MRGS_E_BAD_ARG) -- a host that
 * finishes renders on a worker thread begins them there too, or uses the _geom / _render pair.  All work is enqueued on the
 * caller's hipStream_t (pass torch.cuda.current_stream().cuda_stream); calls on distinct streams/devices are
 * independent.  Return value: 0 on success, otherwise an MRGS_E_* code (mrgs_strerror gives the text);
 * nothing throws across the ABI.
 */
#ifndef MRGS_H_INCLUDED
#define MRGS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRGS_MAX_FEATURES 24 /* cuda_rasterizer/config.h:17 */
#define MRGS_TILE 16         /* cuda_rasterizer/config.h:19-20 */
#define MRGS_NUM_OTHERS 7    /* auxiliary.h:25-29: depth, alpha, normal xyz, median depth, distortion */

enum {
    MRGS_OK = 0,
    MRGS_E_BAD_ARG = 1,       /* shape / pointer contract violated (AT_ERROR in rasterize_points.cu:64-66) */
    MRGS_E_TOO_MANY_FEATURES = 2,
    MRGS_E_NEED_COLORS = 3,   /* neither SH nor precomputed colours (rasterizer_impl.cu:248-251) */
    MRGS_E_HIP = 4,           /* a HIP runtime call failed; see mrgs_last_hip_error() */
    MRGS_E_WORKSPACE = 5,     /* workspace too small for this call */
    MRGS_E_UNSUPPORTED = 6,
    MRGS_E_INTERNAL = 7       /* a bounded device-side wait overran (binning look-back); results were not written */
};

/* Scalar arguments shared by forward and backward; mirrors GaussianRasterizationSettings
 * (diff_surfel_rasterization/__init__.py:167-179) plus the tensor extents the pybind layer derives
 * (rasterize_points.cu:69-72,116-121). */
typedef struct MrgsRasterConfig {
    uint32_t struct_size; /* = sizeof(MrgsRasterConfig) of the header the caller was built against; any other value -> MRGS_E_BAD_ARG
                             (a caller built against another revision of this header is refused instead of being misread) */
    int32_t P;            /* number of gaussians (means3D.size(0)) */
    int32_t S;            /* extra feature channels (features.size(1)), 0..MRGS_MAX_FEATURES */
    int32_t D;            /* active SH degree (raster_settings.sh_degree) */
    int32_t M;            /* SH coefficients per gaussian (sh.size(1)), 0 when colours are precomputed */
    int32_t H, W;         /* image_height, image_width */
    float tanfovx, tanfovy;
    float scale_modifier;
    int32_t prefiltered;
    int32_t debug;        /* nonzero: synchronise the stream and report HIP errors after every kernel (CHECK_CUDA, auxiliary.h:303-310) */
} MrgsRasterConfig;

/* Per-gaussian inputs (device pointers, contiguous fp32, the GaussianModel getter layout):
 * means3D[P,3], shs[P,M,3] or NULL, colors_precomp[P,3] or NULL, features[P,S] (may be NULL when S==0),
 * opacities[P], scales[P,2]+rotations[P,4] (w,x,y,z) or both NULL with transMat_precomp[P,9] given.
 * Camera: viewmatrix[16], projmatrix[16] (row-vector convention tensors, read as stored), campos[3], bg[3]. */
typedef struct MrgsRasterInputs {
    uint64_t struct_size;  /* = sizeof(MrgsRasterInputs); checked like MrgsRasterConfig::struct_size.  The struct has grown optional
                              trailing fields (work_hint, shs_rest, bwd_grad_ws, hint_flags) which the calls ACT on: a shorter struct from
                              an older header would make the library read them past its end */
    const float* bg;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* features;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* transMat_precomp;
    const float* viewmatrix;
    const float* projmatrix;
    const float* campos;
    uint32_t* work_hint;   /* optional, in/out, device, mrgs_work_hint_bytes(H, W), zero-initialised by the caller once per camera: the
                              forward orders its blend waves by the work each (tile, quadrant) took the last time this buffer was
                              passed (falling back to the cull count where it holds 0) and stores the work of this call.  A training
                              loop revisits the same cameras, so the previous visit predicts where rays terminate early far better than
                              any count available before the blend.  NULL: cull counts only.  Results do not depend on its CONTENTS.
                              The buffer also carries the blend kernels' queue state, tickets and the forward's dealt queues
                              (MrgsHintLayout), so (a) renders that share one buffer -- the same camera -- are issued on ONE stream, one
                              after the other (two forwards of one camera on two streams would hand every item out once ACROSS both
                              kernels; renders with different buffers, or without one, are independent on any streams), and (b) a
                              backward that names a prepared workspace (bwd_grad_ws below) is given the SAME buffer its forward was
                              given, not rewritten in between by anything but this library: a fresh or zeroed buffer there makes every
                              wave pull item 0.  The Python wrapper keeps the forward's tensor in the autograd node for that reason. */
    const float* shs_rest; /* optional: split SH layout.  When set, `shs` holds the DC coefficients [P,1,3] and shs_rest the higher orders
                              [P,M-1,3] (M = 2..16) -- the two tensors GaussianModel stores (_features_dc / _features_rest,
                              scene/gaussian_model.py:401-402), which the reference concatenates for every render (get_features,
                              :256-259); MrgsRasterGrads::dL_dsh_rest must then be set too (dL_dsh receives [P,1,3]). */
    void* bwd_grad_ws;     /* optional.  FORWARD calls: the grad_ws (mrgs_grad_bytes) the caller will hand to mrgs_rasterize_backward for
                              this render.  The forward then prepares the backward while it runs anyway -- the gradient rows are cleared by
                              spare workgroups of its ordering launch and the backward's work queues are set up as a copy of its own -- and the
                              backward needs no launch before its blend kernel.  BACKWARD call: pass the same pointer (and the same
                              grad_ws) to say that this was done; NULL, or a pointer other than grad_ws, makes the backward order and clear
                              by itself.  Valid for ONE backward per forward, with the forward's work_hint buffer (above).  Results do not
                              depend on it. */
    uint32_t hint_flags;   /* MRGS_HINT_REUSE_ORDER: the forward skips the ordering of its blend waves and deals them as the last
                              ordering of this camera did -- the dealt queues live in the work_hint buffer, behind the per-block work
                              (mrgs_work_hint_bytes covers both).  Only with work_hint set, and only after a forward WITHOUT the flag has
                              run on the same buffer; the caller (the Python wrapper: every visit of a camera but the first two and every
                              sixteenth) is responsible for that.  A schedule only: results do not depend on it. */
    uint32_t features_live; /* ABI 8 (was reserved, 0): 0 = every one of the S feature channels may be non-zero.  n in 1 .. S - 1: channels n .. S - 1
                               are PADDING (the caller keeps them zero -- e.g. rows of 9 channels padded to 12 floats so that they are 16-byte
                               pieces): the blend kernels leave them out of their per-entry arithmetic, their output maps are written as zeros,
                               their columns of dL_dfeatures stay zero and the upstream gradient of those maps is not read.  Honoured for
                               S = 12 with n = 9 and a 16-byte aligned tensor (the "pgsr" flavour's rows: the blend kernels stage eight channels
                               as for S = 8 and take the ninth from the spare float of the surfel record, where preprocess copies it); any
                               other combination is treated as 0 -- the results are the same, only slower. */
} MrgsRasterInputs;
#define MRGS_HINT_REUSE_ORDER 1u
#define MRGS_HINT_VISIBLE_BYTES 2u   /* ABI 8: `radii` of the forward calls points at P int32 FOLLOWED BY P bytes, and the forward also writes
                                        radii[i] > 0 into byte i of the tail (every render function of the reference returns that mask as
                                        "visibility_filter": a torch kernel per view otherwise) */

/* Workspace sizes.  geom <-> geomBuffer (GeometryState, rasterizer_impl.cu:157-172), img <-> imgBuffer
 * (ImageState, :174-181), binning <-> binningBuffer (BinningState, :183-196; sized from num_rendered). */
size_t mrgs_geom_bytes(int32_t P, int32_t H, int32_t W);
size_t mrgs_img_bytes(int32_t H, int32_t W);
size_t mrgs_binning_bytes(int64_t num_rendered);
size_t mrgs_work_hint_bytes(int32_t H, int32_t W);

/* Forward, phase 1 of 2.  Replaces the first half of CudaRasterizer::Rasterizer::forward
 * (rasterizer_impl.cu:200-291: preprocess, prefix sum, blocking read-back of num_rendered).
 * Writes radii[P] (int32), fills geom_ws, and returns the number of (tile, gaussian) pairs in
 * *num_rendered_host after synchronising `stream` (the reference does the same blocking 4-byte copy, :287). */
int mrgs_rasterize_forward_geom(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, void* geom_ws, size_t geom_bytes,
                                int32_t* radii, int64_t* num_rendered_host, void* stream);

/* Forward, phase 2 of 2.  Replaces rasterizer_impl.cu:293-348 (duplicateWithKeys, tile sort, tile ranges,
 * per-tile blend).  Outputs (caller-allocated; fully written, no pre-zeroing needed): out_color[3,H,W],
 * out_feature[S,H,W], out_others[7,H,W].  binning_ws must hold mrgs_binning_bytes(num_rendered). */
int mrgs_rasterize_forward_render(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, void* geom_ws, void* binning_ws,
                                  size_t binning_bytes, void* img_ws, int64_t num_rendered, float* out_color,
                                  float* out_feature, float* out_others, void* stream);

/* Both phases in one call, without a host round trip in the middle of the GPU work: the binning workspace is carved for
 * `capacity_pairs` (a guess, e.g. the previous call's count plus a margin; binning_bytes >= mrgs_binning_bytes(capacity_pairs)),
 * phase 2 is queued right behind phase 1 and takes the actual pair count from device memory, and the call returns once the
 * count has reached the host (the GPU keeps working).  Returns MRGS_OK with *num_rendered_host set when the count fitted.
 * Returns MRGS_E_WORKSPACE with *num_rendered_host set when it did not: the outputs are then those of an EMPTY render (every tile
 * list reads as empty: background colour, zero maps -- finite, so that work queued behind the call runs on defined data) and the
 * caller redoes phase 2 with mrgs_rasterize_forward_render on a workspace of mrgs_binning_bytes(*num_rendered_host).
 * mrgs_rasterize_backward must be given the pair count the binning workspace was carved for (capacity_pairs here).
 * Same reference interface as the two calls above (rasterize_points.cu:41-144). */
int mrgs_rasterize_forward(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, void* geom_ws, size_t geom_bytes,
                           void* binning_ws, size_t binning_bytes, int64_t capacity_pairs, void* img_ws, int32_t* radii,
                           float* out_color, float* out_feature, float* out_others, int64_t* num_rendered_host, void* stream);

/* The same call in two halves, for callers that have more work to queue behind the rasterizer before they need the count (a renderer
 * queues its per-pixel kernels; the host never sits between the tile scan and the blend): _begin queues both phases and returns at
 * once, _finish waits until the count has reached the host and reports it -- MRGS_OK, or MRGS_E_WORKSPACE exactly as above (everything
 * computed from the outputs is then undefined as well and the caller redoes the view).  A ticket is valid on the host thread that
 * began it until MRGS_TICKET_RING (16) later begins on the same device; a stale one returns MRGS_E_BAD_ARG. */
typedef struct MrgsRasterTicket {
    int32_t device, slot;
    uint64_t seq;
    int64_t capacity_pairs;
} MrgsRasterTicket;
int mrgs_rasterize_forward_begin(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, void* geom_ws, size_t geom_bytes,
                                 void* binning_ws, size_t binning_bytes, int64_t capacity_pairs, void* img_ws, int32_t* radii,
                                 float* out_color, float* out_feature, float* out_others, MrgsRasterTicket* ticket, void* stream);
int mrgs_rasterize_forward_finish(const MrgsRasterTicket* ticket, int64_t* num_rendered_host);

/* Gradient outputs of mrgs_rasterize_backward, the tuple returned by RasterizeGaussiansBackwardCUDA
 * (rasterize_points.cu:146-252): all fully written by the call (no pre-zeroing needed). */
typedef struct MrgsRasterGrads {
    uint64_t struct_size;  /* = sizeof(MrgsRasterGrads); checked like MrgsRasterConfig::struct_size */
    float* dL_dmeans2D;    /* [P,3]  (.xy = densification proxy, backward.cu:665-668; .z = 0) */
    float* dL_dcolors;     /* [P,3] */
    float* dL_dfeatures;   /* [P,S] */
    float* dL_dopacity;    /* [P,1] */
    float* dL_dmeans3D;    /* [P,3] */
    float* dL_dtransMat;   /* [P,9] */
    float* dL_dsh;         /* [P,M,3] */
    float* dL_dscales;     /* [P,2] */
    float* dL_drotations;  /* [P,4] */
    float* dL_dsh_rest;    /* [P,M-1,3] with the split SH layout (MrgsRasterInputs::shs_rest; dL_dsh is then [P,1,3]), else NULL */
    /* ABI 10 -- the glue epilogue: both NULL, or both set by render_surfel's caller (declared further down: the raw GaussianModel parameters
     * and their gradient tensors, the arguments of mrgs_surfel_features_backward).  Set: the per-gaussian backward applies the backward of the
     * per-gaussian glue (gaussian_renderer/__init__.py:338-355 and the GaussianModel getters: sigmoid / exp / normalize) to its results while
     * they are in registers and writes glue_grads' nine tensors (fully; d_indirect_dc / d_indirect_rest as zeros) INSTEAD of dL_dopacity,
     * dL_dscales, dL_drotations, dL_dfeatures and dL_dmeans3D, which are not touched and may be NULL; dL_dcolors and dL_dtransMat are written
     * if not NULL.  One pass over the P rows instead of two (mrgs_surfel_features_backward is not called for this render).
     * Contract: the rows mrgs_surfel_features_forward wrote for the same parameters (scales / rotations given, no precomputed transMat) --
     * S = 8 with glue_params->viewmatrix NULL, or the "pgsr" rows (S = 12, features_live = 9) with the viewmatrix they were built with: the
     * plane distance's gradient then goes to the raw rotation and the centre inside the epilogue (campos = MrgsRasterInputs::campos) --
     * and NO upstream gradient at feature channels 5..7 (nothing reads the blended indirect radiance: render_surfel without opt.indirect),
     * so that the mirror direction takes no gradient.  Other row shapes or a precomputed transMat: MRGS_E_UNSUPPORTED; the three channels'
     * zero gradient is the caller's word (it is not read).  glue_params' indirect_dc / indirect_rest / xyz / campos are not read. */
    const struct MrgsSurfelParams* glue_params;
    const struct MrgsSurfelGrads* glue_grads;
} MrgsRasterGrads;

/* Backward.  Replaces CudaRasterizer::Rasterizer::backward (rasterizer_impl.cu:353-462).  The three
 * workspaces must be the ones the forward of the same view filled.  grad_ws: scratch of
 * mrgs_grad_bytes(P,S) bytes for the packed per-gaussian accumulators. */
size_t mrgs_grad_bytes(int32_t P, int32_t S);
int mrgs_rasterize_backward(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, const int32_t* radii, const void* geom_ws,
                            const void* binning_ws, const void* img_ws, int64_t num_rendered, const float* dL_dout_color,
                            const float* dL_dout_feature, const float* dL_dout_others, void* grad_ws,
                            const MrgsRasterGrads* grads, void* stream);

/* The same backward in two halves (no counterpart in the reference, which is single-process): _blend runs the per-tile blend backward
 * (backward.cu:145-468) and, when dL_dRGB_masked [P,3] is given, writes the colour gradient of every surfel as the SH backward consumes
 * it (zero where the forward clamped the channel, backward.cu:33-36, and for culled surfels) -- final at that point; _finish runs the
 * per-gaussian backward (backward.cu:614-669) and fills `grads`.  A view-parallel step starts its all-gather of dL_dRGB_masked between
 * the two calls (materialrefgs_amd/dist.py: FactoredGradReducer.begin_early), where it overlaps the second half.
 * mrgs_rasterize_backward == _blend(..., NULL) followed by _finish. */
int mrgs_rasterize_backward_blend(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, const int32_t* radii, const void* geom_ws,
                                  const void* binning_ws, const void* img_ws, int64_t num_rendered, const float* dL_dout_color,
                                  const float* dL_dout_feature, const float* dL_dout_others, void* grad_ws, float* dL_dRGB_masked,
                                  void* stream);
int mrgs_rasterize_backward_finish(const MrgsRasterConfig* cfg, const MrgsRasterInputs* in, const int32_t* radii, const void* geom_ws,
                                   const void* grad_ws, const MrgsRasterGrads* grads, void* stream);

/* Replaces markVisible (rasterize_points.cu:254-273, rasterizer_impl.cu:56-68,143-155). present: uint8[P]. */
int mrgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                      void* stream);

/* ---- environment lookup and deferred specular shading ("second boundary") ----------------------
 * The mip chain of scene/light.py:EnvLight: level i is a [6,res_i,res_i,3] fp32 cubemap holding PRE-sigmoid texels
 * (light.py:129); face/orientation convention of cube_to_dir (scene/light_utils.py:24-31).  grad[i] (may be NULL) receives
 * dL/dtexel by atomic accumulation into grad_copies[i] privatised copies -- the caller zero-fills them and sums them. */
#define MRGS_MAX_MIPS 8
typedef struct MrgsEnvMips {
    int32_t n_levels;
    int32_t res[MRGS_MAX_MIPS];
    const float* tex[MRGS_MAX_MIPS];
    float* grad[MRGS_MAX_MIPS];
    int32_t grad_copies[MRGS_MAX_MIPS];   /* >= 1: grad[i] holds this many consecutive copies of the level; workgroups spread
                                             their atomics over the copies (thousands of pixels mirror into each texel of the
                                             coarse levels, and same-address atomics serialise in L2); the caller sums them */
    float min_roughness, max_roughness;   /* EnvLight.min_roughness / max_roughness (0.08 / 0.5) */
} MrgsEnvMips;

/* Replaces EnvLight.__call__(l, roughness=...) (scene/light.py:99-129): out[N,3] = sigmoid(trilinear cube fetch at the mip
 * level get_mip(roughness)).  roughness == NULL selects mode="pure_env" (level 0 only). */
int mrgs_envmap_lookup_forward(const MrgsEnvMips* mips, int64_t N, const float* dirs, const float* roughness, float* out, void* stream);
int mrgs_envmap_lookup_backward(const MrgsEnvMips* mips, int64_t N, const float* dirs, const float* roughness, const float* g_out,
                                float* g_dirs /*[N,3] or NULL*/, float* g_roughness /*[N] or NULL*/, void* stream);

typedef struct MrgsStridedMap { const float* ptr; int64_t stride_h, stride_w, stride_c; } MrgsStridedMap;   /* element strides */
typedef struct MrgsShadeFrame {
    int32_t H, W;
    float Kinv[9];          /* inverse intrinsics, row-major, host values (np.linalg.inv(K), utils/refl_utils.py:64) */
    const float* R;         /* device [3,3]: Camera.R (stored transposed, i.e. camera-to-world rotation) */
    const float* T;         /* device [3]:   Camera.T (world-to-camera translation) */
    MrgsStridedMap albedo;  /* [H,W,3] */
    MrgsStridedMap normal;  /* [H,W,3] world-space shading normal (rend_normal / alpha) */
    MrgsStridedMap alpha;   /* [H,W,1] */
    MrgsStridedMap refl;    /* [H,W,1] refl_strength */
    MrgsStridedMap roughness; /* [H,W,1] */
    const float* lut;       /* device [lut_res, lut_res, 2] split-sum FG table (assets/bsdf_256_256.bin layout, refl_utils.py:9) */
    int32_t lut_res;
} MrgsShadeFrame;

/* Replaces get_specular_color_surfel without visibility tracing (utils/refl_utils.py:364-419): per pixel, in one pass,
 * specular[3,H,W] = direct_light * alpha * specular_weight, direct_light[3,H,W], specular_weight[H,W,3]. */
int mrgs_shade_specular_forward(const MrgsEnvMips* mips, const MrgsShadeFrame* frame, float* specular, float* direct_light,
                                float* specular_weight, void* stream);
/* ... and render_surfel's compositing in the same pass (ABI 6; mrgs_surfel_composite_forward's arithmetic on the specular just computed):
 * diffuse[3,H,W] = (1 - refl) base_color, render[3,H,W] = [linear_to_srgb](diffuse + specular) + bg (1 - alpha).
 * zero_fill / zero_floats (ABI 9): a buffer this launch clears on the side (NULL / 0 = nothing) -- the texel-gradient buffers the
 * backward of this render will accumulate into (mrgs_surfel_shade_composite_backward expects them zeroed and has no launch in front
 * of it that could do it). */
int mrgs_shade_specular_forward_composite(const MrgsEnvMips* mips, const MrgsShadeFrame* frame, const float* base_color, const float* bg,
                                          int32_t srgb, float* specular, float* direct_light, float* specular_weight, float* render,
                                          float* diffuse, float* zero_fill, int64_t zero_floats, void* stream);
/* Gradients w.r.t. the five maps (dense, fully written: g_albedo[H,W,3], g_normal[H,W,3], g_alpha[H,W], g_refl[H,W],
 * g_roughness[H,W]) and, through mips->grad, w.r.t. the cubemap texels (ACCUMULATED into mips->grad: the caller clears them).  Any of
 * the three upstream gradients may be NULL.  A level that receives gradients must have fewer than 2^24 texels (res < 1673; the
 * reference's EnvLight uses 16 ... 128, at most 512): larger ones return MRGS_E_UNSUPPORTED. */
int mrgs_shade_specular_backward(const MrgsEnvMips* mips, const MrgsShadeFrame* frame, const float* g_specular, const float* g_direct_light,
                                 const float* g_specular_weight, float* g_albedo, float* g_normal, float* g_alpha, float* g_refl,
                                 float* g_roughness, void* stream);
/* render_surfel's compositing backward AND the shading backward in ONE launch (ABI 9; gaussian_renderer/__init__.py:436-445 then
 * utils/refl_utils.py:364-419 backwards): what mrgs_surfel_composite_backward followed by mrgs_shade_specular_backward computes, with
 * the compositing's g_specular / g_refl / g_alpha shares kept in the pixel's registers and the per-pixel gradients leaving as the
 * gradient of the rasterizer's [8,H,W] feature map: g_features = (g_refl, g_roughness, g_albedo[3], 0, 0, 0), channel-major.  g_render / g_diffuse [3,H,W]: upstream gradients
 * of the two composited maps (either may be NULL); g_specular_extra [3,H,W]: an upstream gradient of the specular map itself (NULL =
 * none); base_color, specular [3,H,W]: the forward's inputs / output; bg[3].  Outputs, fully written: g_base[3,H,W], g_normal[H,W,3],
 * g_features[8,H,W], g_alpha[H,W] (total).  The texel gradients are accumulated into mips->grad, which must be zero on entry
 * (mrgs_shade_specular_forward_composite's zero_fill clears them in the forward of the same render). */
int mrgs_surfel_shade_composite_backward(const MrgsEnvMips* mips, const MrgsShadeFrame* frame, int32_t srgb, const float* base_color,
                                         const float* specular, const float* bg, const float* g_render, const float* g_diffuse,
                                         const float* g_specular_extra, const float* g_direct_light, const float* g_specular_weight,
                                         float* g_base, float* g_normal, float* g_features, float* g_alpha, void* stream);

/* ---- one-bounce light from the material mesh: RayTracer.secondary_indirect_color (raytracing_brdf/raytracer.py:218-271) -------------
 * One launch, one ray per lane, over the outputs of mrgs_bvh_trace.  Per ray i:
 *   active != NULL and active[i] == 0                          -> out = 0
 *   depth[i] >= 10 (a miss)                                    -> out = sigmoid(level-0 fetch of `base` along -rays_v[i])   (mode="pure_env")
 *   otherwise, with (a, b, c) = the vertices of triangle face_ids[i] and p = hit_pos[i]:
 *     weights  area(p,b,c), area(p,c,a), area(p,a,b) over area(a,b,c), areas of the xy-PROJECTION, absolute values (barycentric_interpolation,
 *              :209-216; evaluated from differences to a); they need not sum to one
 *     diffuse, albedo, metallic m, roughness r, normal n = the weighted rows of `table` (n is NOT normalised)
 *     NdotV = n . v,  l = safe_normalize(2 n NdotV - v),  fg = FG table at clamp((NdotV, r), 0, 1)       -- every ray its OWN pair
 *     light = sigmoid(trilinear fetch of `mips` at get_mip(r) along l)
 *     out   = (1 - m) diffuse + ((0.04 (1 - m) + albedo m) fg0 + fg1) light
 *   a hit whose projected triangle area is exactly 0, or whose face id / vertex ids lie outside the mesh -> out = 0, no gradient.
 * table [n_vertices,12] fp32, 16-byte aligned: diffuse 3, albedo 3, metallic, roughness, normal 3 (decoded: the kernel applies nothing), pad.
 * base [6,base_res,base_res,3]: the un-filtered level EnvLight.base; mips: the prefiltered chain EnvLight.specular.
 * MRGS_E_BAD_ARG before any launch: a wrong struct_size, flags != 0, a negative count, a resolution < 1, and with n_rays > 0 a NULL pointer
 * (only `active` is optional), a mis-aligned table, or n_vertices / n_triangles == 0.  n_rays == 0 -> MRGS_OK, nothing is launched. */
typedef struct MrgsBounceConfig {
    uint32_t struct_size;    /* = sizeof(MrgsBounceConfig); checked like MrgsRasterConfig::struct_size */
    uint32_t flags;          /* 0 */
    int64_t n_rays, n_vertices, n_triangles;
    int32_t base_res, lut_res;
} MrgsBounceConfig;
int mrgs_bounce_shade_forward(const MrgsBounceConfig* cfg, const MrgsEnvMips* mips, const float* base, const float* hit_pos /*[N,3]*/,
                              const float* rays_v /*[N,3]*/, const int32_t* face_ids /*[N]*/, const float* depth /*[N]*/,
                              const uint8_t* active /*[N] or NULL*/, const float* vertices /*[V,3]*/, const int32_t* triangles /*[T,3]*/,
                              const float* table, const float* lut /*[lut_res,lut_res,2]*/, float* out /*[N,3]*/, void* stream);
/* The backward, one launch; it recomputes the gather from the same inputs.  g_out [N,3].  ACCUMULATED by float atomics into buffers the
 * caller zero-fills (each may be NULL = not wanted): g_base (one copy of `base`, miss rays), mips->grad (every level of the chain, hit rays),
 * g_table [n_vertices,8] = diffuse 3, albedo 3, metallic, roughness on the three vertices of the hit triangle (roughness through both the
 * FG table's v coordinate and the mip level).  Nothing flows to positions, directions or the normal attribute. */
int mrgs_bounce_shade_backward(const MrgsBounceConfig* cfg, const MrgsEnvMips* mips, const float* base, float* g_base, const float* hit_pos,
                               const float* rays_v, const int32_t* face_ids, const float* depth, const uint8_t* active, const float* vertices,
                               const int32_t* triangles, const float* table, const float* lut, const float* g_out, float* g_table,
                               void* stream);

/* ---- environment prefilter: EnvLight.build_mips (scene/light.py:72-86) ------------------------------------------------
 * renderutils' specular_cubemap / diffuse_cubemap (scene/renderutils/c_src/cubemap.cu:110-354, ops.py:390-459) are fixed linear
 * operators for a given (resolution, roughness, cos_cutoff): out[t] = sum_s w(t,s) cube[s] / sum_s w(t,s).  They are built
 * once as CSR matrices with normalised weights and applied every iteration as 3-channel SpMVs (forward with the matrix,
 * backward with its transpose, which the caller builds from the CSR).  kind: 0 specular GGX lobe, 1 diffuse cosine.
 * Texel index = (face * res + y) * res + x; cubemaps are [6,res,res,3] fp32.
 *   count: row_count[6 res^2] non-zeros per output texel, row_wsum[6 res^2] = sum of its un-normalised weights
 *   fill:  col / val for row_ptr = exclusive prefix sum of row_count (val = weight / row_wsum for kind 0, the plain weight for kind 1:
 *          diffuse_cubemap is not normalised) */
int mrgs_cubemap_filter_count(int32_t res, int32_t kind, float roughness, float cos_cutoff, uint32_t* row_count, float* row_wsum, void* stream);
int mrgs_cubemap_filter_fill(int32_t res, int32_t kind, float roughness, float cos_cutoff, const uint32_t* row_ptr, const float* row_wsum,
                             uint32_t* col, float* val, void* stream);
/* y[nrows,3] = A x for a CSR matrix A (row_ptr[nrows+1]).  The kernel is bound by streaming A from HBM, so A may be stored
 * compactly: col holds uint16 (col_bytes 2, <= 65536 columns) or uint32 (4) column indices; val holds fp32 weights (val_bytes 4,
 * row_scale may be NULL) or 16-bit fixed-point weights q (val_bytes 2) with weight = q * row_scale[row].  lanes_per_row: 4 for
 * short rows, 64 for rows of hundreds of non-zeros.
 * val_bytes 8 = BLOCKED rows (the long rows of these filters touch runs of consecutive texels): row_ptr counts blocks, col holds the
 * uint16 block index (columns 4 b .. 4 b + 3), val four uint16 fixed-point weights per block (lowest column first; 0 where the row has
 * no entry), weight = q * row_scale[row].  Needs col_bytes 2, lanes_per_row 64, nrows % 4 == 0 (square filters: x has nrows texels), x
 * 16-byte and val 8-byte aligned; MRGS_E_BAD_ARG otherwise. */
int mrgs_csr_spmv3(int32_t nrows, const uint32_t* row_ptr, const void* col, int32_t col_bytes, const void* val, int32_t val_bytes,
                   const float* row_scale, const float* x, float* y, int32_t lanes_per_row, void* stream);
/* Up to MRGS_SPMV_MAX_BATCH independent products of the kind above in ONE launch (`descs` is a host array): the levels of
 * EnvLight.build_mips each way. */
#define MRGS_SPMV_MAX_BATCH 8
#define MRGS_SPMV_MAX_PANEL 1024       /* patches of a tile's panel (image_rows form of MrgsSpmvDesc) */
/* image_rows != NULL (ABI 8) = TILES OF ROWS OF ONE FUNDAMENTAL DOMAIN of the cube's symmetry group, as dense matrices.  The weight
 * of a filter is K(r, c) * area(c) / n(r) with K invariant under the 48 signed axis permutations g of the cube (K(g r, g c) = K(r, c);
 * the reference's texel solid angle, cubemap.cu:17-30, and with it the row sum are not -- they are per-texel factors), so the rows of the
 * texels r0 of a triangle of face 0 (y <= x < res / 2) are the whole operator:
 *     y[image_rows[r0 * 48 + g]] = row_scale[that row] * sum_c W(r0, c) * pre_scale[g c] * x[g c]      (image_rows < 0: skipped)
 * with g c as mrgs_cube_symmetry_rows lists it.  The rows are stored tile by tile (tile t = rows tile_ptr[t] .. tile_ptr[t + 1], at most
 * 16: a 4 x 4 patch of the triangle); panel_src[panel_ptr[t] .. panel_ptr[t + 1]) lists the 4 x 4 texel PATCHES ((face * res / 4 +
 * y / 4) * res / 4 + x / 4) the rows of tile t touch -- the image of a patch under a symmetry is a patch; `val` holds, for every
 * panel patch and each of 64 lanes (lane = 16 * (x & 3) + row in tile), the 16-bit fixed-point weights of the patch's four rows y & 3
 * as one 8-byte word (lowest row first) -- the A operand of v_mfma_f32_16x16x4_f32 as its lanes read it; the 48 symmetries x 3
 * channels are the product's right-hand sides.  nrows = 6 res^2 (the length of x, y, pre_scale, row_scale), res a power of two in
 * 4 .. 128; row_ptr, col, lanes_per_row, col_bytes, val_bytes are not used.  The matrices are 1/40 of the full ones and stay in cache;
 * x is read once per (tile, g). */
typedef struct MrgsSpmvDesc {
    int32_t nrows, lanes_per_row, col_bytes, val_bytes;
    const uint32_t* row_ptr;
    const void* col;
    const void* val;
    const float* row_scale;
    const float* x;
    float* y;
    const int32_t* image_rows;
    const float* pre_scale;
    const uint32_t* tile_ptr;
    const uint32_t* panel_ptr;
    const uint16_t* panel_src;
    int32_t res, n_tiles;
    int32_t max_panel, reserved;   /* the longest panel, in patches: 1 .. MRGS_SPMV_MAX_PANEL */
} MrgsSpmvDesc;
int mrgs_csr_spmv3_batched(const MrgsSpmvDesc* descs, int32_t n, void* stream);
/* rows[g * 6 res^2 + t] = the texel ((face * res + y) * res + x) that the g-th of the cube's 48 symmetries (signed axis permutations,
 * the library's order) maps texel t to; `rows` is a HOST array.  g = 0 is the identity. */
int mrgs_cube_symmetry_rows(int32_t res, int32_t* rows);
/* cubemap_mip applied n_steps times below `in` [6,res_in,res_in,3] (scene/light.py:74-76): outs[k] = level k + 1 ([6, res_in >> (k+1), ., 3]),
 * `outs` a host array of device pointers; bit-identical to n_steps calls of mrgs_cubemap_mip_forward, one launch per three levels.
 * The backward chain g[k] += cubemap_mip.backward(g[k + 1]) for k = n_levels - 2 ... 0 in place (g[k]: [6, res0 >> k, ., 3], g a host
 * array), one launch per level. */
int mrgs_cubemap_mip_chain_forward(int32_t res_in, int32_t n_steps, const float* in, float* const* outs, void* stream);
int mrgs_cubemap_mip_chain_backward(int32_t res0, int32_t n_levels, float* const* g, void* stream);
/* cubemap_mip (scene/light_utils.py:66-81): forward = 2x2 box filter [6,2r,2r,3] -> [6,r,r,3]; backward = the reference's own
 * rule (seamless bilinear cube fetch of 0.25 * dout at the finer level's texel-centre directions), ACCUMULATED into g_fine. */
int mrgs_cubemap_mip_forward(int32_t res_out, const float* in, float* out, void* stream);
int mrgs_cubemap_mip_backward(int32_t res_fine, const float* dout, float* g_fine, void* stream);

/* ---- cubemapencoder fetch primitive (BASELINE.json north star: "the cubemapencoder mip lookup") ---------------------------
 * Replaces `_cubemapencoder.cubemap_encode_forward / cubemap_encode_backward` of the reference's CUDA extension
 * (submodules/cubemapencoder/src/cubemapencoder.cu:430-485, 713-775; bindings.cpp), same argument meaning and layouts:
 * inputs [B,3] directions (a zero vector yields fail_value), cubemap [6,C,L,L], fail_value [C], outputs [C,B];
 * interp 0 = nearest (:380-428), 1 = bilinear; seamless != 0 takes edge texels from the neighbouring face and averages the three
 * texels of a cube vertex (:298-334, face / edge tables :66-187).  Backward: grad_cubemap [6,C,L,L] and grad_fail [C] are ACCUMULATED
 * into (the caller passes zeros, as cubemap_encoder.py:55-57 does), grad_inputs [B,3] is written in full (zeros for nearest, which
 * the reference leaves uninitialised). */
int mrgs_cubemap_encode_forward(const float* inputs, const float* cubemap, const float* fail_value, float* outputs, int32_t interp,
                                int32_t seamless, int64_t B, int32_t C, int32_t L, void* stream);
int mrgs_cubemap_encode_backward(const float* grad_outputs, const float* inputs, const float* cubemap, float* grad_cubemap, float* grad_inputs,
                                 float* grad_fail, int32_t interp, int32_t seamless, int64_t B, int32_t C, int32_t L, void* stream);

/* Visibility blend of get_specular_color_surfel (utils/refl_utils.py:393-401), one pass each way:
 * specular = (direct * vis + (1 - vis) * indirect) * alpha * weight, indirect_color = (1 - vis) * indirect * alpha * weight.
 * direct / specular / indirect_color [3,H,W], weight [H,W,3] (layouts of mrgs_shade_specular_forward), indirect [H,W,3] and alpha
 * [H,W,1] strided maps, visibility [H,W] (constant).  Backward writes g_direct [3,H,W], g_weight [H,W,3], g_indirect [H,W,3],
 * g_alpha [H,W] in full; either upstream gradient may be NULL. */
int mrgs_indirect_blend_forward(int32_t H, int32_t W, const float* direct, const float* weight, const MrgsStridedMap* indirect,
                                const MrgsStridedMap* alpha, const float* visibility, float* specular, float* indirect_color, void* stream);
int mrgs_indirect_blend_backward(int32_t H, int32_t W, const float* direct, const float* weight, const MrgsStridedMap* indirect,
                                 const MrgsStridedMap* alpha, const float* visibility, const float* g_specular, const float* g_indirect_color,
                                 float* g_direct, float* g_weight, float* g_indirect, float* g_alpha, void* stream);

/* g_features[8,H,W] of render_surfel's material map (refl, roughness, albedo[3], indirect[3]) assembled from the outputs of
 * mrgs_surfel_composite_backward (g_refl), mrgs_shade_specular_backward (g_refl, g_roughness [H,W]; g_albedo [H,W,3]) and, with the
 * visibility tracer, mrgs_indirect_blend_backward (g_indirect [H,W,3]; NULL = zeros).  In the same pass g_alpha [H,W] (NULL = skip) receives
 * the sum of the up to three alpha gradients of those kernels (g_alpha_a / _b / _c, each [H,W] or NULL). */
int mrgs_surfel_feature_grads(int32_t H, int32_t W, const float* g_refl_composite, const float* g_refl_shade, const float* g_roughness,
                              const float* g_albedo_hwc, const float* g_indirect_hwc, float* g_features, const float* g_alpha_a,
                              const float* g_alpha_b, const float* g_alpha_c, float* g_alpha, void* stream);

/* ---- per-gaussian inputs of the surfel renderer (fused glue) -----------------------------------------------------
 * One kernel instead of the ~50 torch kernels the reference runs per view before the rasterizer call: GaussianModel getters
 * (scene/gaussian_model.py:236-311: sigmoid / exp / normalize activations), get_normal (:269-285) and the feature assembly of
 * render_surfel (gaussian_renderer/__init__.py:338-355): view direction, facing unit normal (third column of R(q)), mirror
 * direction r = 2 (n.w_o) n - w_o, indirect = clamp_min(eval_sh(3, cat(indirect_dc, indirect_rest), r), 0),
 * features[P,8] = (sigmoid refl, sigmoid roughness, sigmoid ori_color[3], indirect[3]).  All pointers are device pointers to
 * contiguous fp32 tensors in the GaussianModel layout: xyz[P,3], scaling_raw[P,2], rotation_raw[P,4] (w,x,y,z), opacity_raw[P,1],
 * refl_raw[P,1], rough_raw[P,1], ori_color_raw[P,3], indirect_dc[P,1,3], indirect_rest[P,15,3], campos[3]. */
typedef struct MrgsSurfelParams {
    int32_t P;
    const float *xyz, *scaling_raw, *rotation_raw, *opacity_raw, *refl_raw, *rough_raw, *ori_color_raw, *indirect_dc, *indirect_rest,
        *campos;
    /* ABI 7, the "pgsr" flavour (arguments/config.py:1): with viewmatrix set (world_view_transform as stored, 16 floats) the feature rows
     * are TWELVE floats -- channel 8 = get_distance (gaussian_renderer/envgs_renderer.py:30-38: |facing normal . centre| in the camera
     * frame, the plane distance the flavour rasterizes as its last channel, __init__.py:348-357), channels 9..11 = 0 (the row is padded
     * to the blend kernels' 16-byte feature pieces) -- and its gradient joins the normal's and the centre's.  NULL: features[P,8]. */
    const float* viewmatrix;
} MrgsSurfelParams;
typedef struct MrgsSurfelGrads {   /* gradients w.r.t. the raw parameters, same shapes, fully written */
    float *d_xyz, *d_scaling, *d_rotation, *d_opacity, *d_refl, *d_rough, *d_ori_color, *d_indirect_dc, *d_indirect_rest;
} MrgsSurfelGrads;
/* outputs: opacity[P,1], scales[P,2], rotations[P,4] (unit), features[P,8] ([P,12] with MrgsSurfelParams::viewmatrix) -- exactly what
 * GaussianRasterizer is fed */
int mrgs_surfel_features_forward(const MrgsSurfelParams* p, float* opacity, float* scales, float* rotations, float* features,
                                 void* stream);
/* upstream gradients of the four outputs (any may be NULL = zero).  d_xyz = the part that flows through the view and mirror directions
 * + g_xyz_upstream [P,3] (NULL = zero): what reached the centres some other way -- the rasterizer's own dL/dmeans3D --, so that the
 * caller's sum of the two is no kernel of its own (ABI 6; must not alias d_xyz).
 * Where the upstream gradient of the three indirect-radiance channels (g_features[:, 5:8]) is exactly zero for all 64 rows of a wave, the
 * wave writes zeros to d_indirect_dc / d_indirect_rest without reading the coefficients: for FINITE coefficients that is what the chain
 * rule gives; a non-finite coefficient, which the reference's torch chain would turn into a NaN gradient (0 x inf), stays unnoticed
 * there.  d_indirect_rest may have any 4-byte alignment (16-byte aligned tensors take the wide stores). */
int mrgs_surfel_features_backward(const MrgsSurfelParams* p, const float* g_opacity, const float* g_scales, const float* g_rotations,
                                  const float* g_features, const MrgsSurfelGrads* grads, const float* g_xyz_upstream, void* stream);

/* ---- per-gaussian shading of the volume renderer (fused glue) ---------------------------------------------------
 * One kernel instead of the chain of torch ops render_volume runs per view before the rasterizer call (gaussian_renderer/__init__.py:
 * 559-661 with opt.indirect false, utils/refl_utils.py:426-445, scene/light.py:99-129): the GaussianModel getters, get_normal, and
 * get_full_color_volume --
 *   n = facing unit third column of R(q) (facing `campos`), w_o = safe_normalize(rays_o - xyz), NdotV = w_o . n,
 *   rays_refl = safe_normalize(2 n NdotV - w_o),
 *   diffuse  = sigmoid(fetch(diffuse level 0, n)) (1 - refl) ori_color,
 *   specular = sigmoid(trilinear fetch(specular chain, rays_refl, get_mip(roughness))) ((0.04 (1 - refl) + ori_color refl) fg0.x + fg0.y)
 * where fg0 = the FG LUT at (NdotV, roughness).clamp(0, 1) OF GAUSSIAN 0 for every gaussian, as the reference indexes it
 * (refl_utils.py:443).  `campos` (camera_center) and `rays_o` (the origin of sample_camera_rays) are the reference's two differently
 * rounded camera positions; a caller with one passes it twice.  Pointers are device pointers to contiguous fp32 tensors in the
 * GaussianModel layout (MrgsSurfelParams); lut [lut_res,lut_res,2].  viewmatrix (16 floats, world_view_transform as stored; "pgsr") or NULL. */
typedef struct MrgsVolumeParams {
    uint32_t struct_size;    /* = sizeof(MrgsVolumeParams); checked like MrgsRasterConfig::struct_size */
    int32_t P;
    const float *xyz, *scaling_raw, *rotation_raw, *opacity_raw, *refl_raw, *rough_raw, *ori_color_raw, *campos, *rays_o, *lut, *viewmatrix;
    int32_t lut_res;
    int32_t reserved;        /* 0 */
} MrgsVolumeParams;
typedef struct MrgsVolumeGrads {   /* gradients w.r.t. the raw parameters, same shapes, fully written */
    uint64_t struct_size;    /* = sizeof(MrgsVolumeGrads) */
    float *d_xyz, *d_scaling, *d_rotation, *d_opacity, *d_refl, *d_rough, *d_ori_color;
} MrgsVolumeGrads;
/* bytes of the backward's scratch `ws` (8-byte aligned; the backward clears it itself).  The library allocates nothing. */
size_t mrgs_volume_features_ws_bytes(void);
/* outputs: opacity[P,1], scales[P,2], rotations[P,4] (unit), colors_precomp[P,3] = specular + diffuse, features[P,11] = (roughness, refl,
 * diffuse[3], specular[3], ori_color[3]); with viewmatrix features[P,12], channel 11 = get_distance (|facing normal . centre| in the
 * camera frame) -- exactly what render_volume feeds GaussianRasterizer.  `diffuse` is a chain of which level 0 is fetched (no roughness).
 * `features` 16-byte aligned.  MRGS_E_BAD_ARG before any launch: a wrong struct_size, P < 0, lut_res < 1, a malformed chain, with P > 0
 * a NULL input or output.  P == 0: MRGS_OK, nothing launched. */
int mrgs_volume_features_forward(const MrgsVolumeParams* p, const MrgsEnvMips* specular, const MrgsEnvMips* diffuse, float* opacity,
                                 float* scales, float* rotations, float* colors_precomp, float* features, void* stream);
/* The exact derivative (flip sign constant; clamp(0,1) and safe_normalize's clamp_min(1e-20) as torch's): upstream gradients of the five
 * outputs (any may be NULL = zero; g_features 16-byte aligned), g_xyz_upstream [P,3] (NULL = zero) added into d_xyz as in
 * mrgs_surfel_features_backward.  Texel gradients are accumulated into grad / grad_copies of BOTH chains (the caller zero-fills and sums
 * them, as for mrgs_envmap_lookup_backward).  The sum over all rows of dL/dfg0 goes through `ws`; a one-thread launch behind the
 * kernel on the same stream adds its share to row 0's d_xyz, d_rotation and d_rough.  Two launches and a 64-byte clear. */
int mrgs_volume_features_backward(const MrgsVolumeParams* p, const MrgsEnvMips* specular, const MrgsEnvMips* diffuse, const float* g_opacity,
                                  const float* g_scales, const float* g_rotations, const float* g_colors_precomp, const float* g_features,
                                  const MrgsVolumeGrads* grads, const float* g_xyz_upstream, void* ws, size_t ws_bytes, void* stream);

/* ---- per-pixel maps of the surfel renderer (fused glue) ------------------------------------------------------------
 * compute_2dgs_normal_and_regularizations (gaussian_renderer/__init__.py:42-90) + depths_to_points / depth_to_normal
 * (utils/point_utils.py:9-37) + the normal_map of render_surfel (:419-421) in one kernel each way.
 *   view_rot   = world_view_transform[:3,:3] as stored (row-major): rend_normal = view_rot * allmap[2:5]
 *   ray_matrix = c2w[:3,:3] * intrins^-1, ray_origin = c2w[:3,3] with c2w, intrins exactly as depths_to_points builds them:
 *                point(x, y) = surf_depth * (ray_matrix * (x, y, 1)) + ray_origin
 * allmap is the rasterizer's [7,H,W] output.  Outputs: rend_normal[3,H,W], surf_depth[1,H,W], surf_normal[3,H,W] (already
 * multiplied by the detached alpha; NULL = skip, render_surfel(wo_render_img)), normal_map[H,W,3] = rend_normal / max(alpha,
 * 1e-6) (NULL = skip). */
typedef struct MrgsMapsFrame {
    int32_t H, W;
    float view_rot[9], ray_matrix[9], ray_origin[3];
    float depth_ratio;
    /* ABI 7, the "pgsr" flavour (arguments/config.py:1; gaussian_renderer/__init__.py:64-69): with rend_distance set ([H,W], the blended
     * plane distance = the flavour's last feature channel) surf_depth is nan_to_num(rend_distance / -(n . ray)), n = allmap[2:5],
     * ray = ((x - (W - 1) / 2) / pgsr_fx, (y - (H - 1) / 2) / pgsr_fy, 1) -- the depth where the pixel's ray meets the blended plane
     * (allmap[7] of the flavour's rasterizer, which is not in the reference's tree: parity unpinned) -- and surf_normal its finite
     * differences; depth_ratio is then not read.  The backward writes the map's gradient to g_rend_distance ([H,W], may be NULL). */
    float pgsr_fx, pgsr_fy;
    const float* rend_distance;
    float* g_rend_distance;
} MrgsMapsFrame;
int mrgs_surfel_maps_forward(const MrgsMapsFrame* fr, const float* allmap, float* rend_normal, float* surf_depth, float* surf_normal,
                             float* normal_map, float* rend_alpha /*[1,H,W] = allmap[1], NULL = skip*/, float* rend_dist /*[1,H,W] = allmap[6]*/,
                             float* rend_alpha2 /*a second copy of rend_alpha for a second consumer (ABI 6), NULL = skip*/, void* stream);
/* g_allmap[7,H,W] (fully written) from the upstream gradients of the four outputs and of rend_alpha = allmap[1:2] and
 * rend_dist = allmap[6:7], which are plain views in the reference ([1,H,W] each; any of the seven may be NULL = zero). */
int mrgs_surfel_maps_backward(const MrgsMapsFrame* fr, const float* allmap, const float* g_rend_normal, const float* g_surf_depth,
                              const float* g_surf_normal, const float* g_normal_map, const float* g_rend_alpha, const float* g_rend_dist,
                              const float* g_rend_alpha2 /*gradient of the second copy (ABI 6), NULL = zero*/, float* g_allmap, void* stream);

/* render_surfel compositing (gaussian_renderer/__init__.py:436-445): diffuse = (1 - refl) * base, render =
 * [linear_to_srgb]((diffuse + specular)) + bg * (1 - alpha).  base_color / specular / render / diffuse [3,H,W],
 * refl_strength / alpha [1,H,W], bg[3]; all contiguous fp32 device tensors. */
int mrgs_surfel_composite_forward(int32_t H, int32_t W, int32_t srgb, const float* base_color, const float* refl_strength, const float* specular,
                                  const float* alpha, const float* bg, float* render, float* diffuse, void* stream);
int mrgs_surfel_composite_backward(int32_t H, int32_t W, int32_t srgb, const float* base_color, const float* refl_strength,
                                   const float* specular, const float* bg, const float* g_render, const float* g_diffuse, float* g_base,
                                   float* g_refl, float* g_specular, float* g_alpha,
                                   float* zero_fill /*ABI 6: zero_floats floats cleared by the same launch (what the caller's next kernel
                                   accumulates into, e.g. mrgs_shade_specular_backward's texel gradients), NULL / 0 = nothing*/,
                                   int64_t zero_floats, void* stream);

/* ---- training loss of one view (fused) ---------------------------------------------------
 * Replaces calculate_loss (utils/loss_utils.py:142-228) = (1 - lambda_dssim) * l1_loss (:22-23) + lambda_dssim * (1 - ssim)
 * (ssim/_ssim, 11x11 gaussian window sigma 1.5, zero padding, :83-119) + lambda_normal * normal consistency (:166-175) +
 * lambda_dist * mean(rend_dist) (:180-182), and its autograd backward.  image / gt: [C,H,W] (C <= 4), rend_normal /
 * surf_normal: [3,H,W], rend_dist: [H,W], image_weight: [H,W] or NULL.  With image_weight the normal term is
 * mean(image_weight * sum_c |surf - rend|), without it mean(1 - sum_c rend * surf); lambda_normal <= 0 / lambda_dist <= 0
 * switch the terms off (the iteration gates of the reference are the caller's business; the pointers may then be NULL).
 * ws (mrgs_loss_ws_bytes) carries the SSIM derivative maps from forward to backward.
 * out_terms[16] (device): [0] loss, [1] Ll1, [2] ssim, [3] loss0, [4] normal term (unscaled mean), [5] lambda_dist * mean(dist),
 * [6] psnr (utils/image_utils.py psnr, mean over channels), [7..7+C) per-channel mse.  Sums are reduced in a fixed order.
 * out_loss (device scalar, may be NULL) receives the loss as well: a host binding can hand it out as its own tensor.
 * g_loss: device scalar dL/dloss (NULL = 1).  Gradients are written in full (no pre-zeroing by the caller). */
typedef struct MrgsLossConfig {
    int32_t H, W, C;
    float lambda_dssim, lambda_normal, lambda_dist;
} MrgsLossConfig;
size_t mrgs_loss_ws_bytes(int32_t H, int32_t W, int32_t C);
int mrgs_loss_forward(const MrgsLossConfig* cfg, const float* image, const float* gt, const float* rend_normal, const float* surf_normal,
                      const float* rend_dist, const float* image_weight, void* ws, size_t ws_bytes, float* out_terms, float* out_loss,
                      void* stream);
int mrgs_loss_backward(const MrgsLossConfig* cfg, const float* image, const float* gt, const float* rend_normal, const float* surf_normal,
                       const float* image_weight, const void* ws, const float* g_loss, float* g_image, float* g_rend_normal,
                       float* g_surf_normal, float* g_rend_dist, void* stream);

/* ---- per-pixel prior terms of one view (fused) ---------------------------------------------------------------------------------
 * The terms the training scripts add to the loss outside calculate_loss, in three groups; a group is on when its pointers are given
 * and off when they are all NULL (a group with only some of them is MRGS_E_BAD_ARG).  N = H W pixels, all maps contiguous fp32.
 *   normal prior (mono_normal_loss, train_refnerf.py:202-251): surf_normal / rend_normal [3,H,W], prior [N,3] (the monocular normal,
 *     camera space), mask [N] or NULL, Rt[9] HOST floats = the camera's R transposed, row-major (v = Rt x).  With a = normalize(v),
 *     b = normalize(prior), normalize(x) = x / max(|x|, 1e-12): l1 = sum m sum_c |a_c - b_c| / sum m, cos = sum m (1 - a.b) / sum m
 *     (m = 1 without a mask).  Where |v| < 1e-12 the clamp is active: the gradient is g / 1e-12 with no projection term.
 *   mask entropy (train_refnerf.py:1213-1215): rend_alpha [N], alpha_mask [N]; o = clamp(alpha, 1e-6f, (float)(1 - 1e-6)),
 *     -mean(m log o + (1 - m) log(1 - o)); the gradient passes where lo <= alpha <= hi.  alpha_mask may be the same pointer as mask.
 *   ref score (train_refreal.py:1238-1258): refl / rough [N], ref_score [N] uint8 (S = nonzero): a1 = mean_S |refl - 0.9|,
 *     a2 = mean_S |rough - 0.05|, b1 = mean_notS |refl - 0.05|, b2 = mean_notS |0.9 - rough|.
 * out_terms[16] (device): [0..3] l1 and cos of surf_normal, then of rend_normal; [4] entropy; [5..8] a1, a2, b1, b2; [9] sum m;
 * [10] |S|; [11] |not S|; [12] a1 + a2 + b1 + b2 / 2; the rest and the terms of a group that is off are 0.  Divisions are IEEE: an
 * all-zero mask or an empty set gives NaN, as the reference does.  Sums are reduced in a fixed order (no atomics): both calls are
 * bitwise repeatable.  Forward: two launches; backward: one.  No host synchronisation in either call.
 * Backward: fwd_terms = the forward's out_terms (the denominators are read from it on the device); g_terms = HOST table of 16 device
 * scalars, the upstream gradients of out_terms[0..8] and [12] (NULL = 0; the other slots are not read).  Every non-NULL gradient map
 * is written in full (g_surf_normal / g_rend_normal [3,H,W], g_alpha / g_refl / g_rough [N]); a map whose group has no upstream
 * gradient is written as zeros without reading the group's inputs.  Nothing reaches the prior, the masks or ref_score.
 * MRGS_E_BAD_ARG before anything is read: wrong struct_size, H or W <= 0, flags != 0, no group at all, a partial group, a mask
 * without the normal group, a missing or misaligned (16 bytes) or too small workspace, a gradient map of a group that is off. */
typedef struct MrgsPriorConfig {
    uint32_t struct_size;           /* = sizeof(MrgsPriorConfig) */
    int32_t H, W;
    uint32_t flags;                 /* reserved: 0 */
} MrgsPriorConfig;
size_t mrgs_prior_ws_bytes(int32_t H, int32_t W);
int mrgs_prior_terms_forward(const MrgsPriorConfig* cfg, const float* Rt, const float* surf_normal, const float* rend_normal,
                             const float* prior, const float* mask, const float* rend_alpha, const float* alpha_mask, const float* refl,
                             const float* rough, const uint8_t* ref_score, void* ws, size_t ws_bytes, float* out_terms, void* stream);
int mrgs_prior_terms_backward(const MrgsPriorConfig* cfg, const float* Rt, const float* surf_normal, const float* rend_normal,
                              const float* prior, const float* mask, const float* rend_alpha, const float* alpha_mask, const float* refl,
                              const float* rough, const uint8_t* ref_score, const float* fwd_terms, const float* const* g_terms,
                              float* g_surf_normal, float* g_rend_normal, float* g_alpha, float* g_refl, float* g_rough, void* stream);

/* ---- Sobel smoothness terms of one view (fused) ----------------------------------------------------------------------------------
 * smooth_loss (utils/loss_utils.py:124-125; train_refreal.py:1261 on base_color_map * ref_score_image) and first_order_edge_aware_loss
 * (:121-122; calculate_loss :185-197 on rend_normal and surf_depth).  One call evaluates 1..MRGS_SMOOTH_MAX_ITEMS items over the same
 * H x W; all maps contiguous, device pointers.  For a map x [H,W], G_x and G_y are the 3 x 3 Sobel pair divided by 8 with a replicate
 * border (kornia's spatial_gradient, mode "sobel", normalized); only |G| is used.  An item:
 *   data [C,H,W] fp32; mask [H W] uint8 or NULL: a zero entry sets the pixel of every channel to 0 BEFORE the stencil, and the gradient
 *   passes where the entry is nonzero; edge_aware 0 or 1.
 *   plain (edge_aware = 0, C in 1..4):       term = 1 / (C H W) sum_c sum_dir sum_p |G_dir(data_c)(p)|
 *   edge-aware (edge_aware = 1, C in {1, 3}): term = 1 / (3 H W) sum_{c<3} sum_dir sum_p |G_dir(data_c')(p)| exp(-|G_dir(img_c)(p)|), with
 *     img [3,H,W] fp32, given once per call and shared by every edge-aware item; c' = c for C = 3 and 0 for C = 1 (torch's broadcast of the
 *     one map against the image's three channels: the mean runs over 3 H W either way).
 * d|G|/dG = sign(G) with sign(0) = 0: a flat region gets an exactly zero gradient.  Nothing reaches img or the masks.
 * out_terms [n_items] (device).  Sums are reduced in a fixed order (no atomics): both calls are bitwise repeatable.  Forward: two
 * launches; backward: one.  No host synchronisation in either call.
 * Backward: g_terms = HOST table of n_items device scalars, the upstream gradients of out_terms (NULL = 0).  Every non-NULL g_data
 * [C,H,W] is written in full: the adjoint of the clamped stencil, the taps of the padded ring folded into the border texels; zeros for an
 * item whose upstream gradient is NULL, without reading its inputs.  With no g_data at all nothing is launched.
 * MRGS_E_BAD_ARG before anything is read: wrong struct_size, H or W <= 0, flags != 0, n_items outside 1..MRGS_SMOOTH_MAX_ITEMS, an item
 * without data, edge_aware other than 0 / 1, C outside the range of the item's kind, an edge-aware item without img, a missing or
 * misaligned (16 bytes) or too small workspace, no out_terms; in backward no g_terms, or an upstream gradient for an item without g_data. */
#define MRGS_SMOOTH_MAX_ITEMS 4
typedef struct MrgsSmoothConfig {
    uint32_t struct_size;           /* = sizeof(MrgsSmoothConfig) */
    int32_t H, W;
    uint32_t flags;                 /* reserved: 0 */
} MrgsSmoothConfig;
typedef struct MrgsSmoothItem {
    const float* data;
    const uint8_t* mask;            /* nullable */
    float* g_data;                  /* backward only; nullable */
    int32_t C;
    int32_t edge_aware;
} MrgsSmoothItem;
size_t mrgs_smooth_ws_bytes(int32_t H, int32_t W);         /* 0 for sizes the calls refuse */
int mrgs_smooth_terms_forward(const MrgsSmoothConfig* cfg, const float* img, const MrgsSmoothItem* items, int32_t n_items, void* ws,
                              size_t ws_bytes, float* out_terms, void* stream);
int mrgs_smooth_terms_backward(const MrgsSmoothConfig* cfg, const float* img, const MrgsSmoothItem* items, int32_t n_items,
                               const float* const* g_terms, void* stream);

/* ---- multi-view material consistency loss (calc_warp_loss, train_refnerf.py:414-739, train_refreal.py:405-729) ------------------
 * View v and neighbour n, both H x W.  Geometry: every pixel p of v is back-projected through depth_v, projected into n, looked up in
 * depth_n (bilinear, border, align_corners), back-projected and re-projected into v; e = |p' - p|.  valid = inside n (strict bounds,
 * view depth > 0.1) and e < pixel_noise_th; weight_map = exp(-e) on valid pixels, 0 elsewhere.  geo = geo_weight * mean over valid of
 * weight * e (MRGS_WARP_GEO; otherwise 0).  Sampling: min(n_valid, sample_num) distinct valid pixels, uniform, deterministic for
 * (seed, valid set), in ascending pixel order -- or the n_given pixel indices in `samples` (n_given >= 0).  Per sample, a
 * (2 patch_half + 1)^2 patch: the view's maps at integer texels (zeros outside), the neighbour's through the sample's plane homography
 * (bilinear, zeros, align_corners).  out_terms[4] (device): geo, base_weight * base colour term, metallic_weight * L-mean over the
 * kept samples, roughness_weight * the same (NaN for an empty keep set; terms switched off and every term with n_valid = 0 are 0).
 * out_counts[4] (device int32): n_valid, samples, kept samples, 0.  keep = min fg over the patch > 0.99 and keep_v[p] != 0 (NULL: all).
 * cam_v / cam_n: device records of 28 floats, world_view_transform (row-vector form, 16), R (9), T (3) of scene/cameras.py.
 * samples (forward, n_given = -1): if not NULL, receives the drawn pixel indices (sample_num slots; the first out_counts[1] are used).
 * Given samples (n_given >= 0) are the caller's contract, not checked on the device: they must be distinct valid pixels inside the
 * image (a duplicate leaves the slot map to one of its copies and the view-map gradients lose the other; an index outside is read as
 * pixel 0), and n_given = 0 with valid pixels gives a NaN base-colour term (the mean over no sample).
 * The view's material maps take no gradient in the reference (it samples them under torch.no_grad()); g_base_v / g_metal_v /
 * g_rough_v are an optional extra (NULL: not computed).
 * ws (mrgs_warp_loss_ws_bytes) carries the draw and per-sample records from forward to backward.  Backward: g_terms[4] (device) are the
 * upstream gradients of out_terms; every non-NULL gradient map is written in full (depth [H,W], base [3,H,W], metal / rough [H,W]).
 * Nothing reaches normal_v, distance_v, fg_v or the weights.  No host synchronisation in either call. */
#define MRGS_WARP_GEO 1u            /* the geometric term (train_refreal.py returns it) */
#define MRGS_WARP_MATERIAL 2u       /* sampling and the base-colour term (iteration > 10000) */
#define MRGS_WARP_METALLIC 4u       /* directional metallic term (needs MATERIAL) */
#define MRGS_WARP_ROUGHNESS 8u      /* directional roughness term (needs MATERIAL) */
typedef struct MrgsWarpConfig {
    uint32_t struct_size;           /* = sizeof(MrgsWarpConfig); checked like MrgsRasterConfig::struct_size */
    int32_t H, W;
    int32_t sample_num;             /* multi_view_sample_num */
    int32_t patch_half;             /* multi_view_patch_size: 1, 2 or 3 (one 64-lane wave per patch) */
    int32_t n_given;                /* -1: draw on the device; 0 .. sample_num: use `samples` as given */
    uint32_t flags;                 /* MRGS_WARP_* */
    uint32_t seed_lo, seed_hi;
    float fx_v, fy_v, cx_v, cy_v, fx_n, fy_n, cx_n, cy_n;   /* Fx, Fy, Cx, Cy of scene/cameras.py:65-68 */
    float pixel_noise_th, geo_weight, base_weight, metallic_weight, roughness_weight;
} MrgsWarpConfig;
typedef struct MrgsWarpMaps {
    const float* depth_v;           /* surf_depth [H,W] */
    const float* depth_n;
    const float* normal_v;          /* rend_normal [3,H,W] */
    const float* distance_v;        /* rend_distance [H,W] */
    const float *base_v, *metal_v, *rough_v;   /* diffuse_map [3,H,W], refl_strength_map [H,W], roughness_map [H,W] of v */
    const float *base_n, *metal_n, *rough_n;   /* the same of n */
    const float* fg_v;              /* foreground mask of v [H,W] */
    const uint8_t* keep_v;          /* [H,W] not on an edge, or NULL */
    const float *cam_v, *cam_n;     /* device camera records (28 floats) */
} MrgsWarpMaps;
size_t mrgs_warp_loss_ws_bytes(int32_t H, int32_t W, int32_t sample_num, int32_t patch_half);
int mrgs_warp_loss_forward(const MrgsWarpConfig* cfg, const MrgsWarpMaps* maps, int32_t* samples, void* ws, size_t ws_bytes,
                           float* weight_map, float* out_terms, int32_t* out_counts, void* stream);
int mrgs_warp_loss_backward(const MrgsWarpConfig* cfg, const MrgsWarpMaps* maps, const void* ws, const float* weight_map,
                            const float* g_terms, float* g_depth_v, float* g_depth_n, float* g_base_v, float* g_metal_v, float* g_rough_v,
                            float* g_base_n, float* g_metal_n, float* g_rough_n, void* stream);

/* ---- grey-image patch NCC of the same view pair (get_consistency_loss2 over lncc, train_refreal.py:358-395, :707-710) -------------
 * The term train_refreal.py adds to its loss next to the ones above; the only one whose gradient goes through the plane homography,
 * so the only one that reaches rend_normal / rend_distance of the view.  It follows a completed mrgs_warp_loss_forward of the same
 * (cfg, maps) on the same stream and takes that call's workspace and weight map: with MRGS_WARP_MATERIAL it reuses the draw and the
 * stored homographies; without, it runs the same sampler (equal seed and valid set: the draw the material terms would have got; given
 * samples are honoured the same way, and `samples` has the meaning it has there).  maps needs cam_v, cam_n, normal_v, distance_v,
 * metal_v and metal_n whatever the flags.  grey_v / grey_n: [H,W] grey photographs.  Per sample, P = (2 patch_half + 1)^2 taps:
 * r = grey_v at the integer texels (zeros outside), q = grey_n through the homography (bilinear, zeros, align_corners; a non-finite
 * position samples zero); cc = cross^2 / (var_r var_q + 1e-8) from the centred patch sums (the reference's literal sums are the same
 * numbers and cancel on flat patches), ncc = clamp(1 - cc, 0, 2); m = patch mean of metal_v + patch mean of metal_n; a sample is used
 * when ncc < 0.9 and m < 0.4.  out_term[0] = ncc_weight * mean over the used samples of ncc * weight_map (0 where none is used: no
 * host read decides it).  out_counts[2]: samples, used samples.  ref_weight_map [H,W]: 1 - m / 2 at the sample pixels (0 where that
 * is below 0.9), 0 elsewhere.  out_ncc [sample_num] / out_use [sample_num] (either may be NULL): per-sample ncc and the use flag.
 * Backward: g_term[1] (device); g_normal_v [3,H,W] and g_distance_v [H,W] (either may be NULL) are written in full.  Every sample
 * owns its centre pixel, so there are no atomics and both calls are bitwise repeatable.  Nothing reaches the grey images, the metal
 * maps, the weights or the depths.  The forward keeps d ncc / d (normal, distance) per sample (4 floats) in ws, so the backward is
 * one pass over the pixels.  No host synchronisation in either call. */
size_t mrgs_warp_ncc_ws_bytes(int32_t H, int32_t W, int32_t sample_num, int32_t patch_half);
int mrgs_warp_ncc_forward(const MrgsWarpConfig* cfg, const MrgsWarpMaps* maps, const float* grey_v, const float* grey_n,
                          const float* weight_map, const void* warp_ws, size_t warp_ws_bytes, int32_t* samples, void* ws, size_t ws_bytes,
                          float ncc_weight, float* out_term, int32_t* out_counts, float* ref_weight_map, float* out_ncc, uint8_t* out_use,
                          void* stream);
int mrgs_warp_ncc_backward(const MrgsWarpConfig* cfg, const void* warp_ws, const void* ws, float ncc_weight, const float* g_term,
                           float* g_normal_v, float* g_distance_v, void* stream);

/* ---- multi-view reflection score of one view (calc_ref_score, train_refreal.py:782-1001, train_refnerf.py:791-1010) ----------------
 * For every pixel p of view v: how much the photographs of its K neighbours disagree with v's own over a plane-warped patch.  One call
 * handles all K neighbours of the view; `neighbours_dev` is a DEVICE table of K records, read in order.  All views are H x W.
 * A neighbour n is valid at p under the reprojection check of mrgs_warp_loss_forward: p back-projected through depth_v, projected
 * into n (0 < u < W, 0 < v < H, z > 0.1), depth_n read there (bilinear, border, align_corners), back-projected, re-projected into v,
 * and |p' - p| < pixel_noise_th.  Taps t of the (2 patch_half + 1)^2 = P patch: a[c,t] = image_v at the integer texel (zeros
 * outside), s_n[c,t] = image_n through the plane homography of p built from normal_v(p) and distance_v(p) (bilinear, zeros,
 * align_corners, + 1e-10 on the third component; a non-finite position samples zero).  cnt(p) = valid neighbours;
 * score(p) = [cnt > 0] (1/P) sum_t sum_c (sum_{n valid} |s_n[c,t] - a[c,t]|) / (cnt + 1e-8).
 * depth_v, distance_v [H,W]; normal_v, image_v [3,H,W]; cam_v: device record of 28 floats as in MrgsWarpMaps.  score [H,W] float and
 * count [H,W] int32 (may be NULL) are written in full.  Geometry and homography in double, colours in fp32.  No atomics, no
 * workspace, no host synchronisation; neighbours and taps go in a fixed order, so the call is bitwise repeatable.  n_neighbours = 0
 * writes zeros (neighbours_dev may then be NULL).
 * MRGS_E_BAD_ARG before any HIP call: a wrong struct_size, H or W <= 0, H W >= 2^30, patch_half outside 1..4, n_neighbours < 0,
 * an intrinsic or pixel_noise_th that is NaN, fx or fy not > 0, a NULL pointer other than count (and neighbours_dev with K = 0). */
typedef struct MrgsRefScoreConfig {
    uint32_t struct_size;           /* = sizeof(MrgsRefScoreConfig) */
    int32_t H, W;
    int32_t patch_half;             /* 1 .. 4 (the reference uses 4: 81 taps) */
    int32_t n_neighbours;           /* K >= 0 */
    float fx_v, fy_v, cx_v, cy_v;   /* Fx, Fy, Cx, Cy of the view (scene/cameras.py:65-68) */
    float pixel_noise_th;           /* opt.multi_view_pixel_noise_th */
} MrgsRefScoreConfig;
typedef struct MrgsRefScoreNeighbour {
    const float* depth;             /* surf_depth of the neighbour [H,W] */
    const float* image;             /* its photograph [3,H,W] */
    float cam[28];                  /* world_view_transform (16), R (9), T (3) */
    float fx, fy, cx, cy;
} MrgsRefScoreNeighbour;
int mrgs_ref_score(const MrgsRefScoreConfig* cfg, const float* depth_v, const float* normal_v, const float* distance_v,
                   const float* image_v, const float* cam_v, const MrgsRefScoreNeighbour* neighbours_dev, float* score, int32_t* count,
                   void* stream);

/* ---- closest-hit ray queries against a triangle mesh (visibility rays) --------------------
 * Replaces RayTracer(vertices, triangles).trace (submodules/raytracing/raytracing/raytracer.py:8-56,
 * raytracing_brdf/raytracer.py:18-123) = create_raytracer + TriangleBvh4::build / ray_trace_gpu
 * (submodules/raytracing/src/raytracer.cu:20-53, bvh.cu:259-302,526-609,694-720) with Triangle::ray_intersect
 * (include/raytracing/triangle.cuh:27-45): back faces are ignored, hits need 0 <= t < 10, depth = 10 marks a miss.
 * mrgs_bvh_build runs on the HOST (as the reference's build does): vertices [n_vertices,3] f32 and triangles [n_triangles,3] i32
 * are host arrays, the hierarchy is written into blob_host (mrgs_bvh_bytes, position independent); the caller copies the blob
 * to the device once per mesh.  mrgs_bvh_trace: all pointers are device pointers; rays_o / rays_d [n_rays,3], outputs
 * positions / normals [n_rays,3] (may alias rays_o / rays_d: the reference's inplace mode), depth [n_rays], face_ids [n_rays]
 * (index into `triangles`, -1 for a miss; may be NULL). */
size_t mrgs_bvh_bytes(int64_t n_triangles);
int mrgs_bvh_build(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, void* blob_host,
                   size_t blob_bytes);
int mrgs_bvh_trace(const void* blob_dev, int64_t n_triangles, int64_t n_rays, const float* rays_o, const float* rays_d, float* positions,
                   float* normals, float* depth, int32_t* face_ids, void* stream);
/* The visibility block of get_specular_color_surfel (utils/refl_utils.py:379-391) in one launch: per pixel with alpha > 0 the mirror
 * ray of the view direction about `normal` ([H,W,3]) is started at rays_o + surf_depth * rays_cam (un-normalised pixel ray,
 * sample_camera_rays_unnormalize :75-93; Kinv = host inverse intrinsics, R / T = device Camera.R / Camera.T as in MrgsShadeFrame)
 * and visibility[H,W] = 1 if nothing is hit within 10 units (or alpha <= 0), else 0.  No ray buffers, no mask compaction. */
int mrgs_bvh_visibility(const void* blob_dev, int64_t n_triangles, int32_t H, int32_t W, const float* Kinv, const float* R, const float* T,
                        const MrgsStridedMap* normal, const MrgsStridedMap* alpha, const float* surf_depth, float* visibility, void* stream);

/* ---- surfel ray tracer (second half) -----------------------------------------------------------------
 * Replaces the un-vendored OptiX extension `diff_surfel_tracing` behind HardwareRendering (gaussian_renderer/optix_utils.py:14-271):
 * SurfelTracer.build_acceleration_structure(v, f, rebuild) (:76) -> mrgs_surfel_bvh_build, SurfelTracer.forward (:185-197) ->
 * mrgs_surfel_trace_forward, its autograd backward -> mrgs_surfel_trace_backward.  The extension's arithmetic is not in the reference
 * tree: the definition is stated in csrc/mrgs_surfel_trace.hip (2DGS compositing of forward.cu:366-420 along a ray) and restated
 * densely in oracle/surfel_trace_oracle.py; parity with the OptiX binary is unpinned.  All pointers are device pointers except
 * bg_host (3 floats on the host).
 * Build (on the device, every call): quad_vertices [n_surfels,4,3] = the four corners get_disks (:36-66) produces per surfel; blob
 * (mrgs_surfel_bvh_bytes) receives the hierarchy, ws (mrgs_surfel_bvh_ws_bytes) is scratch that may be reused after the call's
 * kernels have run.
 * Trace: ray_o / ray_d [n_rays,3] (direction not normalised: depths are ray parameters); ray_width > 0 says the rays are an image
 * with rows of that length (n_rays a multiple of it): a wavefront then takes an 8x8 block of neighbouring rays instead of 64 of a
 * row (same results, shorter walks); the trace calls write the surfel records in leaf order into the blob (not const); geom [n_surfels,16] per surfel
 * (mean.xyz, a.xyz, b.xyz, n.xyz, opacity, 3 unused) with a = r_u / s_u, b = r_v / s_v, n = r_u x r_v; attr [n_surfels,8] =
 * (rgb, others[2], 3 unused).  Outputs rgb / norm [n_rays,3], dpt / acc / dist [n_rays], aux [n_rays,2], wet [n_surfels] (summed
 * blend weight per surfel, cleared by the call), state [mrgs_surfel_trace_state_floats(n_rays, ray_width)] (per ray: sum w t^2, final transmittance, hits blended, passes -- negative when the ray walked in a packet --; behind them the list of the rays traced one per wavefront and the record of the ids every wavefront gathered, pass by pass, which the
 * backward replays instead of walking the hierarchy again (4 KB per wavefront and pass; when it overflows the backward walks): what the
 * backward needs beyond the outputs).  Backward: g_* of the six outputs in, g_geom [n_surfels,16] / g_attr [n_surfels,8] (cleared by
 * the call, same layout as geom / attr) and g_ray_o / g_ray_d [n_rays,3] out. */
size_t mrgs_surfel_bvh_bytes(int64_t n_surfels);
size_t mrgs_surfel_bvh_ws_bytes(int64_t n_surfels);
size_t mrgs_surfel_trace_state_floats(int64_t n_rays, int32_t ray_width);
/* A state WITHOUT the replay record (the per-ray part and the lists only; ~1/100 of the full size): enough for a forward whose
 * backward will never run (evaluation, torch.no_grad()).  Both trace calls take the size of the state they are handed (state_floats):
 * at least the full size -> the forward records; at least this size -> it does not, and a backward on such a state walks the hierarchy
 * again; smaller -> MRGS_E_WORKSPACE.  n_rays >= 2^31 (or >= 2^27 blocks of rays) -> MRGS_E_UNSUPPORTED.  n_surfels == 0: outputs are
 * the background / zeros, `state` is not touched. */
size_t mrgs_surfel_trace_state_floats_norecord(int64_t n_rays, int32_t ray_width);
/* Introspection for the tests: word offsets inside `state` of [0] the lists of rays traced one per wavefront (their counts, one per
 * XCD region of the launch, at words 0, 64, ..., 448 of the list's 512-word header), [1] the lists of packets handed to the second launch
 * (counts the same way),
 * [2] the record header (word 0: chunks taken from the shared
 * pool, word 1: non-zero = no usable record, the backward walks again), [3] the replay record, [4] the full size. */
int mrgs_surfel_trace_state_layout(int64_t n_rays, int32_t ray_width, size_t* offsets5);
int mrgs_surfel_bvh_build(const float* quad_vertices, int64_t n_surfels, void* blob, size_t blob_bytes, void* ws, size_t ws_bytes, void* stream);
int mrgs_surfel_trace_forward(void* blob, int64_t n_surfels, int64_t n_rays, int32_t ray_width, const float* ray_o, const float* ray_d, const float* geom,
                              const float* attr, const float* bg_host, float* rgb, float* dpt, float* acc, float* norm, float* dist,
                              float* aux, float* wet, float* state, size_t state_floats, void* stream);
int mrgs_surfel_trace_backward(void* blob, int64_t n_surfels, int64_t n_rays, int32_t ray_width, const float* ray_o, const float* ray_d, const float* geom,
                               const float* attr, const float* bg_host, const float* rgb, const float* dpt, const float* acc,
                               const float* norm, const float* aux, const float* state, size_t state_floats, const float* g_rgb, const float* g_dpt,
                               const float* g_acc, const float* g_norm, const float* g_dist, const float* g_aux /* any of the six g_* may be NULL = zeros */,
                               float* g_geom, float* g_attr, float* g_ray_o, float* g_ray_d, void* stream);

/* The per-surfel records of the tracer from the model's tensors, and the way back: what HardwareRendering.render_gaussians prepares
 * around the tracer call (gaussian_renderer/optix_utils.py:36-66 get_disks, :124-183) in one launch each.  scales [P,2] (multiplied by
 * scale_modifier), rotations [P,4] (w,x,y,z; normalised inside as build_rotation does), opacities [P]; exactly one of shs [P,M,3]
 * (colour = max(SH(degree, direction from campos) + 0.5, 0), forward.cu:20-81) and colors_precomp [P,3]; others [P,2] nullable;
 * campos: 3 floats on the device.  quad_vertices [P,4,3] (nullable) receives get_disks' corners for mrgs_surfel_bvh_build.
 * Backward: g_geom [P,16] / g_attr [P,8] in, gradients of every input out (g_shs or g_colors_precomp, g_others nullable). */
int mrgs_surfel_trace_prep_forward(int64_t P, const float* means3D, const float* scales, const float* rotations, const float* opacities,
                                   const float* shs, int32_t M, int32_t sh_degree, const float* colors_precomp, const float* others,
                                   const float* campos, float scale_modifier, float* geom, float* attr, float* quad_vertices, void* stream);
int mrgs_surfel_trace_prep_backward(int64_t P, const float* means3D, const float* scales, const float* rotations, const float* shs, int32_t M,
                                    int32_t sh_degree, const float* campos, float scale_modifier, const float* g_geom, const float* g_attr,
                                    float* g_means3D, float* g_scales, float* g_rotations, float* g_opacities, float* g_shs,
                                    float* g_colors_precomp, float* g_others, void* stream);

/* The same records straight from the model's own tensors (GaussianModel's activations applied inside, scene/gaussian_model.py:56-78,
 * 236-259): scaling_raw [P,2] (scales = exp), rotation_raw [P,4], opacity_raw [P] (opacities = sigmoid), the colour SH split as the model
 * stores it -- features_dc [P,1,3], features_rest [P,15,3] -- and the gradients in the same layout: replaces the getters' ~12 torch
 * kernels (incl. the cat of the two SH tensors) and their ~25 backward kernels per traced view. */
int mrgs_surfel_trace_prep_raw_forward(int64_t P, const float* xyz, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                       const float* features_dc, const float* features_rest, int32_t sh_degree, const float* others,
                                       const float* campos, float scale_modifier, float* geom, float* attr, float* quad_vertices, void* stream);
int mrgs_surfel_trace_prep_raw_backward(int64_t P, const float* xyz, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                                        const float* features_dc, const float* features_rest, int32_t sh_degree, const float* campos,
                                        float scale_modifier, const float* g_geom, const float* g_attr, float* g_xyz, float* g_scaling_raw,
                                        float* g_rotation_raw, float* g_opacity_raw, float* g_features_dc, float* g_features_rest, float* g_others,
                                        void* stream);

/* The mirror rays of a rendered view, as render_indirect / render_surfel_with_envgs set them up (gaussian_renderer/envgs_renderer.py:717-724,
 * __init__.py:496-505): origin = camera centre + surf_depth * un-normalised pixel ray + 1e-3 * direction, direction = unit mirror
 * direction of the view ray about `normal` ([H,W,3], any strides).  Kinv: inverse intrinsics on the host; R / T: device Camera.R /
 * Camera.T as in MrgsShadeFrame.  Backward: gradients of ray_o / ray_d to normal ([H,W,3] contiguous) and surf_depth. */
int mrgs_mirror_rays_forward(int32_t H, int32_t W, const float* Kinv_host, const float* R, const float* T, const MrgsStridedMap* normal,
                             const float* surf_depth, float* ray_o, float* ray_d, void* stream);
int mrgs_mirror_rays_backward(int32_t H, int32_t W, const float* Kinv_host, const float* R, const float* T, const MrgsStridedMap* normal,
                              const float* g_ray_o, const float* g_ray_d, float* g_normal, float* g_surf_depth, void* stream);
/* The same with the reflecting normal built inside from the BLENDED normal map and alpha, as render_surfel_with_envgs does
 * (gaussian_renderer/__init__.py:493-495): normal = safe_normalize(rend_normal / clamp_min(alpha, 1e-6)); rend_normal [H,W,3] by strides
 * (the [3,H,W] map is passed as strides (W, 1, H W)), alpha [H,W].  Backward: + g_alpha [H,W]. */
int mrgs_mirror_rays_blended_forward(int32_t H, int32_t W, const float* Kinv_host, const float* R, const float* T, const MrgsStridedMap* rend_normal,
                                     const float* alpha, const float* surf_depth, float* ray_o, float* ray_d, void* stream);
int mrgs_mirror_rays_blended_backward(int32_t H, int32_t W, const float* Kinv_host, const float* R, const float* T, const MrgsStridedMap* rend_normal,
                                      const float* alpha, const float* g_ray_o, const float* g_ray_d, float* g_rend_normal, float* g_alpha,
                                      float* g_surf_depth, void* stream);
/* out = a (1 - s) + s b per channel: the traced light blended into the rendered view (gaussian_renderer/__init__.py:517).  a / out / g_*
 * [3,H,W] contiguous; b by element strides (channel, pixel: a [H,W,3] tensor seen as [3,H,W] is (1, 3)), s by its pixel stride; backward:
 * g_a [3,H,W], g_b in b's layout, g_s [H,W], all fully written. */
int mrgs_traced_blend_forward(int32_t H, int32_t W, const float* a, const float* b, int64_t b_channel_stride, int64_t b_pixel_stride, const float* s,
                              int64_t s_pixel_stride, float* out, void* stream);
int mrgs_traced_blend_backward(int32_t H, int32_t W, const float* a, const float* b, int64_t b_channel_stride, int64_t b_pixel_stride, const float* s,
                               int64_t s_pixel_stride, const float* g_out, float* g_a, float* g_b, float* g_s, void* stream);


/* ---- optimizer step -------------------------------------------------------------------------
 * torch.optim.Adam(l, lr=0.0, eps=1e-15).step() of GaussianModel.training_setup (scene/gaussian_model.py:417-453) for every
 * parameter tensor in one launch (per MRGS_ADAM_MAX_TENSORS tensors): amsgrad off, no weight decay.  `tensors` is a HOST array;
 * param / grad / exp_avg / exp_avg_sq are device pointers to `numel` contiguous fp32 values (updated in place, grad read only),
 * lr the group's learning rate, step the 1-based count of this update for this tensor (torch keeps one per parameter).
 * beta1 / beta2 / eps are doubles like torch's python scalars: 1 - beta and the bias corrections are formed in double and
 * rounded to fp32 where torch rounds them. */
#define MRGS_ADAM_MAX_TENSORS 32
typedef struct MrgsAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float lr;
    int32_t step;
} MrgsAdamTensor;
int mrgs_adam_step(const MrgsAdamTensor* tensors, int32_t n_tensors, double beta1, double beta2, double eps, void* stream);

/* The same update for the rows a view touched only ("sparse Adam over visible gaussians").  Every tensor is [n_rows, row_floats]
 * (numel == n_rows * row_floats, row_floats <= MRGS_ADAM_ROWS_MAX_WIDTH); masks[0 .. n_masks - 1], 1 <= n_masks <= MRGS_ADAM_ROWS_MAX_MASKS,
 * are device uint8 [n_rows] (bool storage is the same bytes) and a row is VISIBLE when any of them is non-zero there.  `masks` itself
 * is a HOST array.  Visible rows get exactly the update of mrgs_adam_step; param, exp_avg and exp_avg_sq of every other row keep their
 * bits (and are neither read nor written where a whole 16-byte piece of the tensor is invisible).  `step` counts the calls, not the times
 * a row was visible.  bias_correction == 0: step_size = lr and the second moment is used as it is (the plain rule of the 3DGS code base's
 * sparse optimizer); otherwise both corrections are formed from `step` as in mrgs_adam_step.  The whole list is validated before the first
 * launch: a refused call (MRGS_E_BAD_ARG; MRGS_E_UNSUPPORTED for a row wider than the limit or 2^43 elements and more) has moved nothing. */
#define MRGS_ADAM_ROWS_MAX_MASKS 4
#define MRGS_ADAM_ROWS_MAX_WIDTH 32768
typedef struct MrgsAdamRowsTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int32_t row_floats;
    float lr;
    int32_t step;
    int32_t reserved;      /* 0 */
} MrgsAdamRowsTensor;
int mrgs_adam_step_rows(const MrgsAdamRowsTensor* tensors, int32_t n_tensors, int64_t n_rows, const uint8_t* const* masks, int32_t n_masks,
                        int32_t bias_correction, double beta1, double beta2, double eps, void* stream);

/* ---- densify / prune compaction ----------------------------------------------------------------
 * Replaces the ~50 boolean-index calls of _prune_optimizer / prune_points (scene/gaussian_model.py:856-905) -- parameter tensors, their
 * two Adam moments, xyz_gradient_accum / denom / max_radii2D -- by one scan of the keep mask and one gather launch for all tensors.
 * keep: device uint8 [n_rows] (non-zero = keep).  mrgs_compact_count scans it into ws (mrgs_compact_ws_bytes) and writes the number
 * of surviving rows to count_dev (device int64): the caller reads it once, allocates the exact-size destinations and calls
 * mrgs_compact_rows with the same keep / ws.  Rows are fp32 rows of `row_floats` values (any 4-byte type can be passed as such);
 * surviving rows keep their order, like tensor[mask]. */
#define MRGS_COMPACT_MAX_TENSORS 64
typedef struct MrgsCompactTensor {
    const float* src;      /* [n_rows, row_floats] */
    float* dst;            /* [count, row_floats] */
    int32_t row_floats;
} MrgsCompactTensor;
size_t mrgs_compact_ws_bytes(int64_t n_rows);
int mrgs_compact_count(int64_t n_rows, const uint8_t* keep, void* ws, size_t ws_bytes, int64_t* count_dev, void* stream);
int mrgs_compact_rows(int64_t n_rows, const uint8_t* keep, const void* ws, const MrgsCompactTensor* tensors, int32_t n_tensors, void* stream);

/* ---- densify_and_prune and the densification statistics -------------------------------------------------------------------
 * Replaces GaussianModel.densify_and_prune (scene/gaussian_model.py:975-1057: clone + cat, split + cat + prune, final prune) and the two
 * per-iteration statistics lines (add_densification_stats :1059-1061 and `max_radii2D[visibility_filter] = max(...)` of the training
 * loops).  Everything the three stages decide follows per SOURCE row from accum, denom, the two raw scalings and the raw opacity:
 *   g = accum / denom (IEEE, NaN -> 0), s = exp(scaling_raw), o = sigmoid(opacity_raw), t = percent_dense_extent
 *   clone  = |g| >= max_grad and max(s) <= t;          split = g >= max_grad and max(s) > t        (disjoint; max_grad > 0)
 *   gone(x) = o < min_opacity or (world_size_limit > 0 and x > world_size_limit)
 *   original kept: not split and not gone(max(s));      clone emitted: clone and not gone(max(s));
 *   N children emitted: split and not gone(max(s_child)), s_child = exp(log(s / (0.8 N)))
 * (the reference's third prune term, max_radii2D > max_screen_size, reads a vector that densification_postfix has zeroed: it never fires).
 * Output rows: kept originals in row order, then clones in row order, then child 0 of every split row in row order, then child 1, ...
 *
 * mrgs_densify_classify writes a class byte per row and the per-block offsets of the three segments into ws (mrgs_densify_ws_bytes) and
 * {n_keep, n_clone, n_child} (n_child = split rows with surviving children, i.e. children per k) to counts_dev (device int64[3]).  The
 * caller reads those 24 bytes once -- the only synchronisation --, allocates destinations of n_keep + n_clone + N n_child rows and calls
 * mrgs_densify_emit with the same cfg / ws and the counts: one launch per MRGS_COMPACT_MAX_TENSORS tensors streams every source once.
 * Roles: COPY every output row is its source row; MOMENT kept originals are copied, every new row is zero; XYZ ([.,3]) a child gets
 * xyz + R(normalize(rotation_raw)) (s_x z0, s_y z1, 0); SCALING ([.,2]) a child gets log(exp(scaling_raw) / (0.8 N)).
 * z0, z1: noise[(row * N + k) * 2 + {0,1}] when `noise` (device fp32 [P,N,2], indexed by SOURCE row) is given; otherwise Philox4x32-10
 * with key (seed low word, seed high word) and counter (row low word, row high word, k, 0): with x0, x1 its first two output words,
 * u_i = ((x_i >> 8) + 1) 2^-24 in (0, 1], z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1).  Stateless, independent
 * of the grid, nothing drawn for rows that are not split.
 * Codes, all before any launch: MRGS_E_BAD_ARG for a wrong struct_size, P < 0, N outside 1..8, max_grad not > 0, a NULL pointer with
 * P > 0 (a dst may be NULL when the three counts are zero: an empty destination has no address), ws too small or not 4-byte aligned, row_floats outside 0..2^20, an XYZ row not 3 or a SCALING row not 2 wide, negative counts or counts beyond P;
 * MRGS_E_UNSUPPORTED when P max(2, N) >= 2^31; P = 0 returns MRGS_OK, launches nothing and writes nothing (counts_dev included). */
#define MRGS_DENSIFY_COPY 0
#define MRGS_DENSIFY_MOMENT 1
#define MRGS_DENSIFY_XYZ 2
#define MRGS_DENSIFY_SCALING 3
typedef struct MrgsDensifyConfig {
    uint32_t struct_size;            /* = sizeof(MrgsDensifyConfig); checked like MrgsRasterConfig::struct_size */
    int32_t N;                       /* children per split row, 1..8 (the reference: 2) */
    int64_t P;                       /* rows before the call */
    float max_grad, min_opacity, percent_dense_extent;
    float world_size_limit;          /* 0.1 * extent when max_screen_size is truthy, <= 0: that term is off */
    const float* xyz_raw;            /* [P,3]  read by mrgs_densify_emit when a table entry has role XYZ */
    const float* scaling_raw;        /* [P,2]  ... role XYZ or SCALING */
    const float* rotation_raw;       /* [P,4]  (w,x,y,z), un-normalised; role XYZ */
} MrgsDensifyConfig;
typedef struct MrgsDensifyTensor {
    const float* src;      /* [P, row_floats] */
    float* dst;            /* [n_keep + n_clone + N n_child, row_floats] */
    int32_t row_floats;
    int32_t role;          /* MRGS_DENSIFY_* */
} MrgsDensifyTensor;
size_t mrgs_densify_ws_bytes(int64_t P);
int mrgs_densify_classify(const MrgsDensifyConfig* cfg, const float* accum, const float* denom, const float* scaling_raw,
                          const float* opacity_raw, void* ws, size_t ws_bytes, int64_t* counts_dev, void* stream);
int mrgs_densify_emit(const MrgsDensifyConfig* cfg, const void* ws, const int64_t* counts_host, const MrgsDensifyTensor* tensors,
                      int32_t n_tensors, uint64_t seed, const float* noise, void* stream);
/* For rows with visible[i] != 0: accum[i] += ||grad[i, 0:3]||_2 (all three columns, as the reference's line), denom[i] += 1 and, when
 * radii and max_radii are both given, max_radii[i] = max(max_radii[i], (float)radii[i]).  In place, one launch, nothing read back.
 * grad fp32 [P,3], visible bytes [P], radii int32 [P] or NULL, accum / denom / max_radii fp32 [P] (max_radii may be NULL). */
int mrgs_densify_stats(int64_t P, const float* grad, const uint8_t* visible, const int32_t* radii, float* accum, float* denom,
                       float* max_radii, void* stream);

/* ---- EnvGaussianModel.densify_and_prune and add_densification_stats (scene/env_gaussian_model.py:384-603) --------------------------
 * The six-stage chain of the environment set in classify passes over per-row numbers and ONE emit pass; no intermediate copy of a
 * parameter tensor exists.  Per source row i (fp32): a = accum, d = denom, r = max_radii, w = weight_accum, s = exp(scaling_raw),
 * m = max(s), o = sigmoid(opacity_raw), t = percent_dense_extent.  Literal to the reference, its quirks included:
 *   1 clone   g = a / d (IEEE, NaN -> 0); clone iff |g| >= max_grad and m <= t.  A clone copies every parameter and a, d, r; its
 *             weight is w * W0, W0 = max of w over the P rows (QUIRK: densify_stats multiplies by xyz_weight_accum.max(), :388).
 *   2 split   over the P + clones rows: split iff m > t and g >= max_grad (QUIRK: a clone carries its source's g, but m <= t, so with
 *             split_screen_threshold None -- the only value served: MRGS_ENV_DENSIFY_SPLIT_SCREEN in flags is MRGS_E_UNSUPPORTED --
 *             clones never split).  Two children: raw scaling log(s / 1.6), xyz + R(normalize(rot)) (s_x z0, s_y z1, 0), radius
 *             r * fl32(1 / 1.6), d copied, weight w * W1 with W1 = max of the weights over the rows before the split, clones included.
 *             Sources are removed.
 *   3 opacity rows with o < min_opacity go.
 *   4 scene / screen   over the n rows now present: wavg = weight / d (IEEE, NaN -> 0), q = their 0.1 quantile (rule below),
 *             big = (MRGS_ENV_DENSIFY_SCREEN and radius > max_screen_size) or m_row > world_size_limit (a child's m_row is exp of the raw
 *             scaling it was given), low = wavg < q.  big and low: pruned.  big and not low: replaced by FIVE children with divisor 2.5,
 *             the same formulas, weight * W4, W4 = max of the weights over the rows left after this stage's prune, the sources about to
 *             be split included.  A stage-2 child split here compounds both offsets and both scalings.
 *   5 cap     with more than n_after rows present, the rows - n_after rows of smallest wavg go.  TIES: among equal wavg (-0 = +0) the
 *             row earlier in the output order goes first (torch.topk leaves ties unspecified: this rule is this library's).
 *   6 reset   the caller zeroes the four statistics vectors at the new length.
 * Zero rows after stage 3 end the call with zero rows (the reference would raise inside torch.quantile).
 * Quantile, every operation a single fp32 rounding: rank = 0.1f * (float)(n - 1), lo = floor(rank), hi = ceil(rank), f = rank - lo, v_lo /
 * v_hi the exact order statistics, q = v_lo + f (v_hi - v_lo) if f < 0.5 else v_hi - (v_hi - v_lo)(1 - f): torch's fp32 quantile / lerp up
 * to whether torch fuses the multiply-add; to the last ulp it is this library's.  The weight path (w, W0, W1, W4, the products, wavg, q,
 * the cut) and the radius path are single IEEE multiplies / divides / maxima / compares.  NaN in weight_accum is not served.
 * Output order: kept slot rows -- unsplit originals, clones, stage-2 child 0, child 1, each in source-row order --, then the stage-4
 * children child-major (child j of every split slot row in that same order, j = 0..4); stage 5 removes rows without reordering.
 * Roles as MrgsDensifyTensor's: COPY; MOMENT travels with surviving originals and is zero for every clone and child; XYZ, SCALING up to
 * two generations.  z of stage-2 child k: noise[(row * 2 + k) * 2 + {0,1}] or Philox4x32-10 as mrgs_densify_emit, counter (row lo, row
 * hi, k, 0); of stage-4 child j of slot sigma (0 original, 1 clone, 2 + k stage-2 child k): noise4[((row * 4 + sigma) * 5 + j) * 2 +
 * {0,1}] or counter (row lo, row hi, j, 1 + sigma).
 * Host reads: ONE.  mrgs_env_densify_classify queues every pass (the selections take k from device memory) and writes
 * MRGS_ENV_DENSIFY_COUNTS int64 to counts_dev: [0,24) rows per output segment (kept slot sigma: sigma; stage-4 child j of slot sigma:
 * 4 + 4 j + sigma), [24] their sum, [25] rows cloned by stage 1, [26] rows split by stage 2, [27] n, [28] / [29] slot rows pruned / split
 * by stage 4, [30] rows removed by stage 5, [31] float bits of q, [32..34] of W0, W1, W4, [35] of the stage-5 cut, [36] rows before
 * stage 5, [37] stage 5 ran.  The caller reads them once, allocates counts[24]-row destinations and calls mrgs_env_densify_emit.
 * Workspace: mrgs_env_densify_ws_bytes(P) = 8192 + align256(40 P) + align256(4 P) + 2 align256(96 ceil(P / 256)) bytes (ten keys and a
 * record per row, sized for the 10 P-row worst case; two [24][blocks] matrices), 256-byte aligned.  No allocation, no synchronisation.
 * Codes, all before any launch: MRGS_E_BAD_ARG for a wrong struct_size, P < 0, n_after < 0, max_grad not > 0, unknown flags, a NULL
 * pointer with P > 0 (a dst may be NULL when n_rows is 0), ws too small or misaligned, n_rows outside 0..10 P, a bad tensor entry as
 * mrgs_densify_emit; MRGS_E_UNSUPPORTED for MRGS_ENV_DENSIFY_SPLIT_SCREEN and for 10 P >= 2^31; P = 0 returns MRGS_OK and launches nothing. */
#define MRGS_ENV_DENSIFY_SCREEN 1u        /* max_screen_size is given (not None) */
#define MRGS_ENV_DENSIFY_SPLIT_SCREEN 2u  /* split_screen_threshold is given: not served */
#define MRGS_ENV_DENSIFY_COUNTS 40
typedef struct MrgsEnvDensifyConfig {
    uint32_t struct_size;            /* = sizeof(MrgsEnvDensifyConfig) */
    uint32_t flags;                  /* MRGS_ENV_DENSIFY_* */
    int64_t P;                       /* rows before the call */
    int64_t n_after;                 /* int(max_gs * max_gs_threshold) */
    float max_grad, min_opacity, percent_dense_extent;
    float world_size_limit;          /* 0.1 * extent */
    float max_screen_size;           /* read with MRGS_ENV_DENSIFY_SCREEN */
    float reserved;
    const float* xyz_raw;            /* [P,3]  read by mrgs_env_densify_emit when a table entry has role XYZ */
    const float* scaling_raw;        /* [P,2] */
    const float* rotation_raw;       /* [P,4]  (w,x,y,z), un-normalised */
} MrgsEnvDensifyConfig;
size_t mrgs_env_densify_ws_bytes(int64_t P);
int mrgs_env_densify_classify(const MrgsEnvDensifyConfig* cfg, const float* accum, const float* denom, const float* max_radii,
                              const float* weight_accum, const float* scaling_raw, const float* opacity_raw, void* ws, size_t ws_bytes,
                              int64_t* counts_dev, void* stream);
int mrgs_env_densify_emit(const MrgsEnvDensifyConfig* cfg, const void* ws, int64_t n_rows, const MrgsDensifyTensor* tensors,
                          int32_t n_tensors, uint64_t seed, const float* noise, const float* noise4, void* stream);
/* The selection both stages use, on its own: the k-th smallest (k from 0) of n fp32 values by a radix select over the order-preserving
 * integer image of the float, 8-bit digits, histograms in LDS, one global add per non-empty bin and block; -0 and +0 are one value, NaN
 * is not served.  out_dev (device uint32[4]): float bits of the value, how many values are smaller, how many are equal, k.  ws:
 * mrgs_env_select_ws_bytes() bytes, 256-byte aligned.  MRGS_E_BAD_ARG: n < 0, n >= 2^31, k outside [0, n), a NULL pointer, ws too small;
 * n = 0 returns MRGS_OK and launches nothing. */
size_t mrgs_env_select_ws_bytes(void);
int mrgs_env_select(int64_t n, const float* values, int64_t k, void* ws, size_t ws_bytes, uint32_t* out_dev, void* stream);
/* EnvGaussianModel.add_densification_stats (:600-603).  For rows with visible[i] != 0: accum[i] += ||grad[i, 0:3]||_2, denom[i] += 1 and,
 * when weight_accumulate is given, weight_accum[i] += weight_accumulate[i].  In place, one launch, nothing read back; max_radii2D is not
 * touched (the reference's update_env_gs never updates it).  MRGS_E_BAD_ARG: P < 0, a NULL pointer with P > 0 (weight_accumulate may be
 * NULL; weight_accum then too). */
int mrgs_env_densify_stats(int64_t P, const float* grad, const uint8_t* visible, const float* weight_accumulate, float* accum, float* denom,
                           float* weight_accum, void* stream);

/* View-parallel training (materialrefgs_amd/dist.py): sum over V views of the SH colour gradients from each view's masked colour
 * gradient dRGB_v = dL/dsh_v[:,0,:] / SH_C0 and camera centre: dL_dsh[p][k][c] = sum_v B_k(normalize(means3D[p] - campos_v)) dRGB_v[p][c]
 * for k < (D+1)^2, 0 beyond (backward.cu:22-141).  gathered = V rows of row_stride floats, row v = [dRGB_v (P x 3) | campos_v (3)]
 * -- the layout an all-gather of the per-rank rows produces.  Replaces the all-reduce of the [P,M,3] gradient (16x the bytes). */
int mrgs_sh_grad_expand(int32_t P, int32_t M, int32_t D, int32_t V, const float* means3D, const float* gathered, int64_t row_stride,
                        float* dL_dsh, void* stream);

/* The same exchange for render_surfel's parameter set (BASELINE config 5): colour SH along the view direction and indirect-radiance SH
 * (eval_sh(3, .) along the mirror direction of the facing normal, gaussian_renderer/__init__.py:338-352) are both rank one per view.
 * gathered row v = [dRGB_v (P x 3) | dIND_v (P x 3) | campos_v (3)] with dRGB_v = d features_dc_v / SH_C0 and
 * dIND_v = d indirect_dc_v / SH_C0; xyz [P,3] and rotation_raw [P,4] (w,x,y,z, un-normalised) are the replicated parameters the
 * directions are rebuilt from.  Writes the summed gradients of features_dc [P,1,3], features_rest [P,15,3] (coefficients beyond
 * (D+1)^2 zero), indirect_dc [P,1,3], indirect_rest [P,15,3]: 96 of the 111 gradient floats per gaussian never cross the links. */
int mrgs_sh_grad_expand_surfel(int32_t P, int32_t D, int32_t V, const float* xyz, const float* rotation_raw, const float* gathered,
                               int64_t row_stride, float* g_features_dc, float* g_features_rest, float* g_indirect_dc, float* g_indirect_rest,
                               void* stream);
/* The same expansion with the three parts of a rank's row in buffers of their own (V rows each, strides in floats): dRGB_v is final after
 * the blend backward and dIND_v only after the per-gaussian backward, so a view-parallel step gathers them at different times
 * (materialrefgs_amd/dist.py: SurfelGradReducer.begin_early_rgb / begin_early_ind) and expands from where the two all-gathers left them.
 * rgb_rows NULL or ind_rows NULL (not both): that family is left out and its two output tensors are not touched (they may be NULL) --
 * one call per family, each as soon as its rows have arrived.  ABI 7. */
int mrgs_sh_grad_expand_surfel_rows(int32_t P, int32_t D, int32_t V, const float* xyz, const float* rotation_raw, const float* rgb_rows,
                                    int64_t rgb_stride, const float* ind_rows, int64_t ind_stride, const float* campos_rows, int64_t campos_stride,
                                    float* g_features_dc, float* g_features_rest, float* g_indirect_dc, float* g_indirect_rest, void* stream);

/* ---- initial scales of a point cloud ---------------------------------------------------------------------------------------
 * Replaces simple_knn's distCUDA2 (submodules/simple-knn/simple_knn.cu:147-221, spatial.cu:14-26), called by
 * GaussianModel.create_from_pcd (scene/gaussian_model.py:367, env_gaussian_model.py:147): out[i] = mean of the squared distances from
 * points[i] to its three nearest OTHER points (other by index: a duplicate at another index is a neighbour at distance 0).
 * A squared distance is (dx dx + dy dy) + dz dz in fp32, un-fused; out[i] = ((b0 + b1) + b2) / 3.0f over the three smallest, a missing
 * neighbour counting as FLT_MAX (P = 1, 2: +inf; P = 3: ~1.1e38): a pure function of the input, bitwise repeatable, invariant under a
 * permutation of the rows and bit-equal to the float32 brute force (the reference, compiled with nvcc's contraction, may differ by an
 * ulp).  Any extent is served, zero on one, two or three axes included.  Rows with a non-finite coordinate, and their neighbours, get
 * unspecified values; the call still completes inside its buffers.
 * points [P,3] and out [P] are device pointers; ws (mrgs_knn_ws_bytes(P) <= 64 P + 1 MiB bytes, 16-byte aligned, contents arbitrary:
 * the call clears what it needs) is scratch that may be reused once the call's kernels have run.  Everything is queued on `stream`;
 * nothing is read back to the host.  MRGS_E_BAD_ARG (before any HIP call): P < 0, P >= 2^31, or a null / misaligned pointer with
 * P > 0; MRGS_E_WORKSPACE: ws_bytes too small; P = 0 returns MRGS_OK and launches nothing.  mrgs_knn_ws_bytes is 0 outside
 * 0 <= P < 2^31. */
size_t mrgs_knn_ws_bytes(int64_t P);
int mrgs_knn_mean_dist2(const float* points, int64_t P, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- ball query, furthest point sampling and the 3D max-pooling of the reflection score -------------------------------------------
 * Replaces pointnet2_ops' ball_query and furthest_point_sample (a CUDA-only extension the reference imports at
 * utils/ref_score_utils.py:1 and does not carry) and the pooling of ref_scores_max_pooling / ref_scores_max_pooling_wiht_mask
 * (utils/ref_score_utils.py:21-121).  The definitions restate pointnet2_ops' published kernels and are what is pinned
 * (tests/pool_statement.py); parity with the CUDA binary is unpinned, its contracted distances may differ in the last bit.
 *   d(q, k) = (dx dx + dy dy) + dz dz in fp32, un-fused, dx = fl(q.x - p_k.x), ...; r = radius, r2 = fl(r r); k HITS q iff d(q, k) < r2
 *   (strictly; a comparison with a NaN is false, so a row with a non-finite coordinate never hits and is never hit).
 *
 * mrgs_ball_query: idx [B,M,nsample] int32; with h_0 < h_1 < ... the hits of query j of new_xyz [B,M,3] among xyz [B,N,3] in ascending
 * index order and c = min(#hits, nsample), row j is h_0 .. h_{c-1} followed by h_0 repeated, all zeros without a hit (and with N = 0):
 * a pure function of the inputs, bit-equal to the fp32 brute force over k = 0 .. N-1.
 *
 * mrgs_ball_max_pool: pooled [B,N]; pooled[j] = the maximum of score[k] (the first hit's score, then fmaxf with each further one) over
 * the row mrgs_ball_query(r, nsample, points, points) would hold for j -- the first nsample hits, not all -- without that row ever
 * existing.  r = radius, or fl(*radius_dev * radius) when radius_dev (one device float, read by the kernel: no host read) is given.
 * valid NULL: a row without a hit takes score[0] of its batch, as the zero row does.  valid [B,N] bytes: rows whose byte is 0 are neither
 * candidates nor queries and keep their own score; the order among the others is their order in the full cloud; a valid row without
 * a hit keeps its own score.
 *
 * mrgs_furthest_point_sample: idx [B,npoint] int32; idx[0] = 0, temp[k] = 1e10; for each further pick every k whose magnitude
 * (x x + y y) + z z (fp32) is > 1e-3 (compared in double: the published kernel's test, kept) is eligible and takes
 * temp[k] = fminf(temp[k], d(p_old, p_k)) with p_old the pick before; the pick is the eligible k of largest temp[k], ties to the lowest
 * index (this library's rule; the CUDA kernel's tie depends on its block size), 0 without an eligible point.  One launch per pick,
 * each reading the pick before from device memory.  span_out (optional, [B] device floats): |p[idx[0]] - p[idx[1]]|, the square root
 * of d correctly rounded; 0 when npoint < 2.
 *
 * mrgs_depth_points: points [n_views H W, 3]; point v H W + y W + x is ((x - cx) / fx z, (y - cy) / fy z, z) with z = depth[y W + x] of
 * view v, then (p - T) @ R^T (R row-major): utils/ref_score_utils.py:8-19 with scale = 1 over scene/cameras.py:96-104.  One launch for
 * all views; `views` is a device array.
 *
 * All pointers are device pointers.  ws (mrgs_ball_query_ws_bytes(B, N) bytes -- one size serves the three calls that take it: 16 B N
 * plus 33 bytes per 64 points -- 16-byte aligned, contents arbitrary) is scratch that may be reused once the call's kernels have run.
 * Everything is queued on `stream`; nothing is read back to the host and nothing is allocated.  Before any HIP call: MRGS_E_BAD_ARG for
 * B < 0, B > 65535 (batches are grid.y), N or M outside [0, 2^31), nsample < 1, npoint < 0, n_views outside [0, 65535], H or W < 0,
 * n_views H W >= 2^31, a null pointer that would be used, a misaligned ws, or N = 0 with a pick to make; MRGS_E_WORKSPACE for ws_bytes
 * too small.  An empty input (B = 0, M = 0, N = 0 for the pooling, npoint = 0, n_views H W = 0) returns MRGS_OK and launches nothing.
 * mrgs_ball_query_ws_bytes is 0 outside those ranges. */
typedef struct MrgsDepthView {
    const float* depth;      /* device fp32 [H, W] */
    float R[9];              /* the camera's R (scene/cameras.py:85), row-major */
    float T[3];
    float fx, fy, cx, cy;
} MrgsDepthView;
size_t mrgs_ball_query_ws_bytes(int64_t B, int64_t N);
int mrgs_ball_query(float radius, int32_t nsample, const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t M, int32_t* idx, void* ws,
                    size_t ws_bytes, void* stream);
int mrgs_furthest_point_sample(const float* xyz, int64_t B, int64_t N, int32_t npoint, int32_t* idx, float* span_out, void* ws, size_t ws_bytes,
                               void* stream);
int mrgs_depth_points(const MrgsDepthView* views, int32_t n_views, int32_t H, int32_t W, float* points, void* stream);
int mrgs_ball_max_pool(float radius, const float* radius_dev, int32_t nsample, const float* points, const float* score, const uint8_t* valid, int64_t B,
                       int64_t N, float* pooled, void* ws, size_t ws_bytes, void* stream);

/* ---- mesh extraction: TSDF fusion, marching tetrahedra, floater removal -----------------------------------------------------
 * Replaces the in-loop mesh step of the training scripts (utils/mesh_utils.py: extract_mesh_bounded :212-253, extract_mesh_unbounded
 * :309-404, post_process_mesh :30-51; utils/mcube_utils.py).  Everything is queued on `stream`; nothing is allocated by the library.
 *
 * mrgs_tsdf_fuse: the rule of compute_unbounded_tsdf / compute_sdf_perframe (:322-373).  Per sample x: tsdf = 1, w = 1; for each view
 * in table order: clip = [x, 1] @ proj (proj row-major [4][4], the camera's full_proj_transform), z = clip.w, ndc = clip.xy / z; the
 * view contributes iff -1 < ndc.x, ndc.y < 1 and z > 0; d = bilinear tap of the view's depth map [H, W] at ndc (align_corners, border
 * padding); when depth_trunc > 0 the view is skipped unless all four texels lie in (0, depth_trunc]; sdf = d - z, contributes iff
 * sdf > -trunc; t = clamp(sdf / trunc, -1, 1); tsdf = (tsdf w + t) / (w + 1); w += 1.  ONE launch per call: the view table is a device
 * array of any length, the view loop runs inside the kernel, the field is written once, w only to weight_debug when that is given.
 * Samples: MRGS_TSDF_PLAIN the lattice x = origin + spacing * (i0, i1, i2), field index (i0 n1 + i1) n2 + i2; MRGS_TSDF_CONTRACTED the same
 * lattice read as contracted coordinates s: x = center + radius * uncontract(s), uncontract(s) = s for |s| < 1, else s / ((2 - |s|) |s|),
 * and trunc times 1 / (2 - min(|s|, 1.9)) where |s| > 1; MRGS_TSDF_POINTS x = points[n_points, 3] as given.
 * Codes, before any launch: MRGS_E_BAD_ARG for a wrong struct_size, an unknown mode, a lattice axis below 2, trunc not > 0, radius not
 * > 0 in contracted mode, n_views < 0, n_points < 0, a NULL field / points / (with n_views > 0) view table; MRGS_E_UNSUPPORTED for 2^39
 * samples or more (the launch's grid); n_points = 0 returns MRGS_OK and launches nothing.  n_views = 0 is served: the field is all 1. */
#define MRGS_TSDF_CONTRACTED 0
#define MRGS_TSDF_PLAIN 1
#define MRGS_TSDF_POINTS 2
typedef struct MrgsTsdfView {
    float proj[16];          /* full_proj_transform, row-major */
    const float* depth;      /* device fp32 [H, W] */
    int32_t H, W;
} MrgsTsdfView;
typedef struct MrgsTsdfConfig {
    uint32_t struct_size;    /* = sizeof(MrgsTsdfConfig) */
    int32_t mode;            /* MRGS_TSDF_* */
    int32_t n0, n1, n2;      /* lattice points per axis (lattice modes) */
    int32_t n_views;
    int64_t n_points;        /* MRGS_TSDF_POINTS */
    float origin[3], spacing[3];
    float center[3], radius; /* MRGS_TSDF_CONTRACTED */
    float trunc;             /* contracted mode: the value inside the unit ball, 5 voxels in the reference */
    float depth_trunc;       /* > 0: texel validity as above; <= 0: off */
    const float* points;     /* device fp32 [n_points, 3] */
} MrgsTsdfConfig;
int mrgs_tsdf_fuse(const MrgsTsdfConfig* cfg, const MrgsTsdfView* views_dev, float* field, float* weight_debug, void* stream);

/* mrgs_vertex_fuse: colour and material maps fused onto points (mesh vertices) -- the "texturing" pass of extract_mesh_unbounded,
 * compute_unbounded_tsdf(..., return_rgb=True) over compute_sdf_perframe (:322-373, called at :402).  Per point x (fp32, as given):
 * a[c] = 0 for every channel c < channels, w = w0.  For each view in table order the acceptance is exactly mrgs_tsdf_fuse's: clip =
 * [x, 1] @ proj, z = clip.w, ndc = clip.xy / z; accepted only if -1 < ndc.x, ndc.y < 1 and z > 0; tap position p = clamp((ndc + 1) / 2 *
 * (S - 1), 0, S - 1) (S = W for x, H for y), its four corners under border padding; with depth_trunc > 0 all four depth texels must lie in
 * (0, depth_trunc]; the weights w00 = (1-tx)(1-ty), w01 = tx(1-ty), w10 = (1-tx)ty, w11 = tx ty are formed once, d = d00 w00 + d01 w01 +
 * d10 w10 + d11 w11, sdf = d - z, accepted only if sdf > -trunc.  If accepted, for every channel s[c] = a00 w00 + a01 w01 + a10 w10 +
 * a11 w11 (the same four weights, in that order) and a[c] = (a[c] w + s[c]) / (w + 1); after all channels w += 1.  A point in front of the
 * seen surface (large positive sdf) contributes, as in the reference: there is no other occlusion test.
 * w0 = 1 is the reference's texturing rule (its weights start at 1 and its rgbs at 0: after k accepted views the value is sum / (k + 1));
 * w0 = 0 is the plain mean, 0 where no view accepts (the bounded mode, where the reference delegates to Open3D: parity unpinned).  No
 * other w0 is served.  out [n_points, channels] holds a, weight [n_points] (or NULL) the final w.
 * The attribute maps are channel-last fp32 [H, W, channels], channels a multiple of 4 (pad with anything: channels do not mix), and
 * 16-byte aligned.  Those pointers live in device memory where this call cannot see them: the caller guarantees the alignment (the
 * Python layer does; a misaligned map faults).  ONE launch per call, whatever the number of views; no atomics: bitwise repeatable.
 * Codes, before any HIP call: MRGS_E_BAD_ARG for a wrong struct_size, channels not in {4, 8, 12, 16}, w0 not in {0, 1}, trunc not > 0,
 * n_views < 0, n_points < 0, NULL points or out with n_points > 0, a NULL table with n_views > 0, out not 16-byte aligned;
 * MRGS_E_UNSUPPORTED for 2^39 points or more (the launch's grid, as mrgs_tsdf_fuse).  n_points = 0 returns MRGS_OK and launches nothing.
 * n_views = 0 is served: out is 0 and weight is w0. */
typedef struct MrgsAttrView {
    float proj[16];          /* full_proj_transform, row-major */
    const float* depth;      /* device fp32 [H, W] */
    const float* attr;       /* device fp32 [H, W, channels], channel-last, 16-byte aligned */
    int32_t H, W;
} MrgsAttrView;
typedef struct MrgsVertexFuseConfig {
    uint32_t struct_size;    /* = sizeof(MrgsVertexFuseConfig) */
    int32_t n_views;
    int64_t n_points;
    int32_t channels;        /* 4, 8, 12 or 16 */
    int32_t w0;              /* 0 or 1 */
    float trunc;
    float depth_trunc;       /* > 0: texel validity as above; <= 0: off */
} MrgsVertexFuseConfig;
int mrgs_vertex_fuse(const MrgsVertexFuseConfig* cfg, const MrgsAttrView* views_dev, const float* points, float* out, float* weight,
                     void* stream);

/* Marching tetrahedra over the lattice of `field` [n0, n1, n2] (index (i0 n1 + i1) n2 + i2, point origin + spacing * (i0, i1, i2)).
 * Every cube is cut into the six Kuhn tetrahedra (c, c+e_a, c+e_a+e_b, c+e_a+e_b+e_c); a point is inside iff F < level; a vertex sits on
 * every lattice edge (3 axes, 3 face diagonals, the body diagonal) whose ends differ, at p_a + (level - F_a) / (F_b - F_a) (p_b - p_a) with
 * a the end of lower lattice index; triangles are wound so that their normal points from inside to outside.  With `contracted` the
 * vertices are then mapped by center + radius * uncontract(.) and clipped to +-32 (mcube_utils.py:91-93).  Vertices are indexed by their
 * owning lattice point, so triangles share indices by construction.
 * The lattice is worked in slabs of `slab_planes` cube layers along axis 0 (ws, mrgs_mesh_ws_bytes, holds one word per point of a slab).
 * mrgs_mesh_count writes {V, T} to totals_dev (device int64[2]); the caller reads those 16 bytes, allocates vertices fp32 [V,3] and
 * triangles int32 [T,3] and calls mrgs_mesh_emit with the same cfg / field / ws.  Vertices are ordered by (lattice index of the owning point, direction
 * code 4 d0 + 2 d1 + d2 of the edge), whatever the slab height; the order of the triangles is unspecified but the same from call to call.
 * Codes, before any HIP call: MRGS_E_BAD_ARG for a wrong struct_size, an axis below 2, slab_planes < 1, a spacing not > 0, a NaN level,
 * radius not > 0 with `contracted`, a NULL field / ws / totals, ws not 8-byte aligned, negative totals, a NULL destination with a
 * non-zero total; MRGS_E_WORKSPACE for ws_bytes too small; MRGS_E_UNSUPPORTED for a slab of more than 2^28 points or a total beyond
 * 2^31 - 1.  Zero totals: mrgs_mesh_emit returns MRGS_OK, launches nothing, and the destinations may be NULL. */
typedef struct MrgsMeshConfig {
    uint32_t struct_size;    /* = sizeof(MrgsMeshConfig) */
    int32_t n0, n1, n2;
    int32_t slab_planes;     /* cube layers per slab, >= 1 */
    int32_t contracted;
    float level;
    float origin[3], spacing[3];
    float center[3], radius;
} MrgsMeshConfig;
size_t mrgs_mesh_ws_bytes(const MrgsMeshConfig* cfg);     /* 0 for a configuration the calls below refuse */
int mrgs_mesh_count(const MrgsMeshConfig* cfg, const float* field, void* ws, size_t ws_bytes, int64_t* totals_dev, void* stream);
int mrgs_mesh_emit(const MrgsMeshConfig* cfg, const float* field, void* ws, size_t ws_bytes, const int64_t* totals_host, float* vertices,
                   int32_t* triangles, void* stream);

/* post_process_mesh (:30-51).  mrgs_mesh_clusters: labels[v] (device int32 [V]) = the smallest vertex index of v's connected component,
 * components through shared vertex indices; counts[l] (device int32 [V]) = triangles of the component whose label is l, 0 elsewhere.
 * mrgs_mesh_select: keep_vertex[v] = counts[labels[v]] >= threshold, keep_triangle[t] likewise through its first corner -- the masks
 * for mrgs_compact_count / mrgs_compact_rows, which keep the survivors' order.  mrgs_mesh_reindex: with new_to_old[V_new] (the old
 * indices of the surviving vertices, e.g. an index column compacted with them) writes remap_ws[old] = new (device int32 [V_old] scratch)
 * and rewrites triangles [T,3] in place.  A corner outside [0, V) is ignored by all three.
 * Codes, before any launch: MRGS_E_BAD_ARG for negative sizes, V_new > V_old, a NULL pointer that would be read or written;
 * MRGS_E_UNSUPPORTED beyond 2^31 - 1; empty inputs return MRGS_OK and launch nothing. */
int mrgs_mesh_clusters(int64_t V, int64_t T, const int32_t* triangles, int32_t* labels, int32_t* counts, void* stream);
int mrgs_mesh_select(int64_t V, int64_t T, const int32_t* triangles, const int32_t* labels, const int32_t* counts, int32_t threshold,
                     uint8_t* keep_vertex, uint8_t* keep_triangle, void* stream);
int mrgs_mesh_reindex(int64_t V_old, int64_t V_new, const int32_t* new_to_old, int32_t* remap_ws, int64_t T, int32_t* triangles,
                      void* stream);

/* The edge mask of the multi-view loss (dilated_edges_imgs, utils/image_utils.py:109-116: cv2.Canny + cv2.dilate on the 8-bit normal map),
 * defined here in integers -- parity with a particular OpenCV build is not claimed:
 *   1 quantise  v = img * 255 (one fp32 multiply), u = trunc(v) as int32, & 255 (negative values wrap: -0.5 -> -127 -> 129); a v that is
 *               not finite or has |v| >= 2^31 gives 0
 *   2 grey      g = (9798 R + 19235 G + 3735 B + 16384) >> 15
 *   3 Sobel     3 x 3, replicate border on g: dx = (g[y-1,x+1] + 2 g[y,x+1] + g[y+1,x+1]) - (the same at x-1), dy = (row y+1: g[x-1] +
 *               2 g[x] + g[x+1]) - (row y-1); m = |dx| + |dy|, 0 outside the image
 *   4 thresholds  low = floor(min(thres1, thres2)), high = floor(max(thres1, thres2))
 *   5 non-maximum suppression  ax = |dx|, ay = |dy| << 15, t22 = ax * 13573, t67 = t22 + (ax << 16); a pixel with m > low is a CANDIDATE
 *               if ay < t22: m > m[y,x-1] and m >= m[y,x+1]; else if ay > t67: m > m[y-1,x] and m >= m[y+1,x]; else, with s = -1 where
 *               dx and dy differ in sign and +1 otherwise: m > m[y-1,x-s] and m > m[y+1,x+s].  A candidate with m > high is STRONG
 *   6 hysteresis  a candidate is an edge exactly if its 8-connected component of candidates holds a strong pixel
 *   7 dilate    a = dilate_size / 2; out[y,x] = OR of edge[y+oy, x+ox] over oy, ox in [-a, dilate_size - 1 - a], positions outside the
 *               image ignored
 *   8 result    out as 0 / 1; with invert, 1 - out (the loss's keep mask)
 * img [3,H,W] fp32, out [H,W] bytes, classes_out (nullable) [H,W] bytes: 0 none, 1 candidate, 2 strong.  Device pointers, the caller's
 * workspace (mrgs_edges_ws_bytes, 256-byte aligned; its contents are scratch) and stream: four launches, nothing is allocated or read
 * back and the call does not synchronise, so it may be captured into a graph.  The result is a set: no value depends on the order of
 * the atomics of the component labelling.
 * Codes, before any HIP call: MRGS_E_BAD_ARG for H or W <= 0, dilate_size outside 1..31, a NaN threshold, a NULL img, out or ws;
 * MRGS_E_UNSUPPORTED for H W >= 2^31; MRGS_E_WORKSPACE for ws_bytes below the size query's answer (0 for sizes the call refuses). */
size_t mrgs_edges_ws_bytes(int32_t H, int32_t W);
int mrgs_edge_mask(const float* img, int32_t H, int32_t W, int32_t dilate_size, float thres1, float thres2, int32_t invert, uint8_t* out,
                   uint8_t* classes_out, void* ws, size_t ws_bytes, void* stream);

/* Introspection used by the parity tests: copies of internal state in the reference's layouts.
 * which: 0 depths f32[P], 1 means2D f32[P,2], 2 transMat f32[P,9], 3 normal_opacity f32[P,4], 4 rgb f32[P,3],
 * 5 tiles_touched u32[P], 6 clamped u8[P,3], 7 point_list u32[R], 8 ranges u32[tiles,2], 9 final_T f32[3,H,W],
 * 10 n_contrib u32[2,H,W], 11 depth-sorted gaussian order u32[P], 12 pixels the forward re-rendered exactly u32[2 + H W] ([0] their
 * count, from [2] their indices), 13 quadrant masks of the tile lists u8[R] (which 8x8 blocks of its tile an entry's box touches),
 * 14 the block-cull records f32[P,12] (centre, A, C | B/C, B/A, det/C, det/A | mean2D, r^2 of the low-pass disc, bound of the centre's
 * error -- csrc/mrgs_blend_math.h: CullConic; tools/cull_model.py restates them on the CPU).
 * dst is a device pointer. */
int mrgs_debug_export(const MrgsRasterConfig* cfg, const void* geom_ws, const void* binning_ws, const void* img_ws,
                      int64_t num_rendered, int32_t which, void* dst, void* stream);

/* The two look-back primitives of the binning on their own, for the tests (tests/test_sort_scan.py); production paths do not go through
 * these.  All pointers but the workspace sizes' are device pointers.  Both calls clear their workspace, synchronise the stream and
 * return MRGS_E_INTERNAL if a look-back gave up.  Before any HIP call: MRGS_E_BAD_ARG for a NULL pointer (n_dev excepted), n < 0,
 * bit_lo < 0, bit_hi > 32, bit_lo >= bit_hi with n > 0, a scan workspace that is not 8-byte aligned; MRGS_E_UNSUPPORTED for n >= 2^30
 * (the scan: n > 2^30); MRGS_E_WORKSPACE for ws_bytes below the size query's answer.
 * mrgs_debug_radix_sort_pairs: stable sort of the n (key, value) pairs on key bits [bit_lo, bit_hi) in place; the other key bits ride
 * along and take no part in the order.  n_dev (nullable): the count is read from the device, n is the capacity; a count above n means
 * "nothing to do" and leaves keys / vals unspecified.
 * mrgs_debug_scan_tiles: offsets[i] = sum of tiles_touched[order[j]] for j < i, *total = the whole sum, saturated at 0xFFFFFFFF (the
 * offsets are then meaningless).  The sum of any 2 048 consecutive terms must stay below 2^32. */
size_t mrgs_debug_sort_ws_bytes(int64_t n);
int mrgs_debug_radix_sort_pairs(uint32_t* keys, uint32_t* vals, int64_t n, const uint32_t* n_dev, int32_t bit_lo, int32_t bit_hi, void* ws,
                                size_t ws_bytes, void* stream);
size_t mrgs_debug_scan_ws_bytes(int64_t n);
int mrgs_debug_scan_tiles(const uint32_t* tiles_touched, const uint32_t* order, int32_t n, uint32_t* offsets, uint32_t* total, void* ws,
                          size_t ws_bytes, void* stream);

/* HIP-event timing of the last forward_render / backward call's dominant kernels on their stream (bench.py). */
typedef struct MrgsKernelTimes {
    float preprocess_ms, sort_ms, duplicate_ms, render_fwd_ms, render_bwd_ms, preprocess_bwd_ms;
} MrgsKernelTimes;
int mrgs_set_profiling(int32_t level);   /* 0 off, 1 every stage, 2 only the two blend kernels, 3 the backward blend kernel on every
                                            fourth call (an event pair costs two ~6 us bubbles on the stream) */
int mrgs_get_kernel_times(MrgsKernelTimes* out);

const char* mrgs_strerror(int code);
/* "<hipGetErrorString> at <file>:<line>" of the most recent MRGS_E_HIP returned to the CALLING thread, by whichever entry point: every
 * such return records its reason first.  Valid until that thread's next failing call (a success does not clear it); "" if the thread
 * has had none. */
const char* mrgs_last_hip_error(void);
const char* mrgs_version(void);

/* Revision of this header's struct layouts and call signatures; a binding compares it with the MRGS_ABI_VERSION it was written
 * against before the first call (materialrefgs_amd/_lib.py does).  Entry points that come or go do not move it: revision 10 has lost
 * the four side-stream calls and the feature-map form of the shading backward, and a binding that still names one of them fails at
 * symbol lookup. */
#define MRGS_ABI_VERSION 10
int32_t mrgs_abi_version(void);

/* GaussianModel's reset family and its normal-propagation step (scene/gaussian_model.py:532-722) in ONE launch: for up to
 * MRGS_RESET_MAX_ITEMS parameter groups the new raw values and, where the optimizer has stepped, both Adam moments written 0 for EVERY
 * row (replace_tensor_to_optimizer, :840-854).  All tensors are device fp32, row-major [P,width]; a dst never aliases any src, so the
 * items of one call all read the values from before the call (a fused step equals the sequence of its single methods as long as no item
 * writes what another item's rule or keep mask reads -- true of the three steps the training loops run).
 * Keep mask: `keep` is an OR of MRGS_RESET_KEEP_*; a row for which ANY selected condition holds copies its src bits to dst unchanged.
 *   EXCLUSIVE    exclusive[row] != 0
 *   REFL_ABOVE   sigmoid(refl_raw[row]) > refl_thr        REFL_BELOW   sigmoid(refl_raw[row]) < refl_thr
 *   ROUGH_ABOVE  sigmoid(rough_raw[row]) > rough_thr
 * The decisions compare the fp32 sigmoid 1 / (1 + expf(-x)) with the fp32 threshold, as the reference does -- not the raw value with
 * logit(thr).  Rules (v a src element, s = that sigmoid of v, L(x) = log(x / (1 - x)) taken in double on the host from the caller's
 * double and rounded once to fp32; af, bf = a, b rounded to fp32; every fp32 operation un-fused, in the order written):
 *   CAP           s > af ? L(a) : v                         reset_opacity0 (a = 0.01)
 *   FLOOR         s < af ? L(a) : v                         reset_refl, reset_refl_strength2
 *   LIFT          s > af ? v : L(a)                         reset_opacity1 (a = 0.9)
 *   CONST         L(a)                                      reset_refl_strength, reset_roughness
 *   FILL          af                                        reset_features
 *   JITTER        v + ((u af) 2 - af)                       dist_color, dist_albedo (a = 0.4)
 *   JITTER_CONST  logf(c / (1 - c)), c = clamp(af + (u - 0.5) bf, 0, 1)      reset_ori_color (0.5, 0.05)
 *   ENLARGE       log(exp(v) af) taken in double from the fp32 v, rounded once      enlarge_refl_scales(ret_raw=True) / reset_scale
 * On the unchanged side of CAP / FLOOR / LIFT the row keeps v bit for bit (the reference writes logit(sigmoid(v)) there: v up to a round
 * trip that loses e^|v| 2^-24 and becomes +-inf from |v| ~ 16.6 on).
 * u: item.noise[row, column] when given, else Philox4x32-10 with key `seed` and counter (row low word, row high word, column, item
 * index), u = (x0 >> 8) 2^-24 in [0, 1).
 * Codes, all before any HIP call: MRGS_E_BAD_ARG for a wrong struct_size, n_items outside 1..MRGS_RESET_MAX_ITEMS, P < 0, width < 1, an
 * unknown rule or unknown keep bits, one moment pointer without the other, a KEEP_* bit whose source pointer is NULL, a NULL src or dst
 * with P > 0, a outside (0, 1) where L(a) is taken; MRGS_E_UNSUPPORTED for width > 2^20 or more than 2^31 - 1 blocks of 256 rows.
 * P == 0 returns MRGS_OK and launches nothing.  One launch, nothing allocated or read back, no synchronisation. */
#define MRGS_RESET_MAX_ITEMS 8
enum { MRGS_RESET_CAP = 0, MRGS_RESET_FLOOR = 1, MRGS_RESET_LIFT = 2, MRGS_RESET_CONST = 3, MRGS_RESET_FILL = 4, MRGS_RESET_JITTER = 5,
       MRGS_RESET_JITTER_CONST = 6, MRGS_RESET_ENLARGE = 7 };
enum { MRGS_RESET_KEEP_EXCLUSIVE = 1, MRGS_RESET_KEEP_REFL_ABOVE = 2, MRGS_RESET_KEEP_REFL_BELOW = 4, MRGS_RESET_KEEP_ROUGH_ABOVE = 8 };
typedef struct MrgsResetItem {
    const float* src;          /* [P,width] raw values, read only */
    float* dst;                /* [P,width] new raw values (never aliases any src) */
    float* exp_avg_dst;        /* [P,width] written 0 for EVERY row, or NULL (optimizer has not stepped) */
    float* exp_avg_sq_dst;     /* both NULL or both set */
    const float* noise;        /* [P,width] uniforms in [0,1) for the JITTER rules, or NULL: Philox */
    int32_t width, rule, keep, reserved;
    double a, b;
} MrgsResetItem;
typedef struct MrgsResetConfig {
    uint32_t struct_size;      /* = sizeof(MrgsResetConfig) */
    int64_t P;
    const float* refl_raw;     /* [P] raw _refl_strength, needed by KEEP_REFL_* */
    const float* rough_raw;    /* [P] raw _roughness,     needed by KEEP_ROUGH_ABOVE */
    const uint8_t* exclusive;  /* [P] or NULL */
    float refl_thr, rough_thr;
    uint64_t seed;
} MrgsResetConfig;
int mrgs_model_reset(const MrgsResetConfig* cfg, const MrgsResetItem* items, int32_t n_items, void* stream);

/* ---- LPIPS (VGG16) perceptual distance of one image pair (lpipsPyTorch/modules: networks.py:88-96, lpips.py:30-36, utils.py:6-8) -----
 * Network: thirteen 3 x 3 convolutions (pad 1, bias, ReLU): 3-64, 64-64 | 64-128, 128-128 | 128-256, 256-256, 256-256 | 256-512,
 * 512-512, 512-512 | 512-512, 512-512, 512-512, a 2 x 2 / stride 2 maximum (floor) at every `|`; stage s works on (H >> s) x (W >> s).
 * Taps: the ReLU outputs of convolutions 2, 4, 7, 10 and 13.  Input: a = in_scale x + in_offset, then (a - shift_c) / scale_c with shift
 * (-.030, -.088, -.188), scale (.458, .448, .450); the padding ring of the first convolution is 0 in that space.  Head: per level and
 * pixel u = f / (sqrt(sum_c f_c^2) + 1e-10) for both images, term_l = mean over the level's pixels of sum_c w_c (u_c - v_c)^2; the
 * result is the sum of the five.  DIFFERENCE to torch: a pixel whose feature vector is all zero in either image contributes 0 and gets
 * gradient 0 (torch's sqrt backward yields NaN there, and its forward counts the other image's vector alone).
 * fp32 throughout: a product sum is an fmaf chain over each chunk of 16 input channels (144 products, on the f32-input matrix
 * instructions), the chunk sums added in order; one plain fmaf chain in the two 3-channel layers.  No
 * float atomics: every sum has a fixed order, the same call twice gives the same bits.  No host read or synchronisation in any call.
 * Images x, y: [3,H,W] fp32 planes.  Activations inside the workspace are channel-last [H_s][W_s][C].
 *
 * Weights: mrgs_lpips_pack_weights reads torch-layout device tensors (conv_w[i] [Cout,Cin,3,3], conv_b[i] [Cout], lin_w[l] [C_l]) and
 * writes ONE blob of mrgs_lpips_weights_bytes() (117.7 MB; 256-byte aligned): per convolution the forward matrix [9][Cin][Cout], the bias,
 * and the matrix of the backward-to-data pass [9][Cout][Cin] with the taps flipped; then the five lin vectors.
 * Workspace: mrgs_lpips_ws_bytes(H, W, with_grad), 0 for sizes the calls refuse; 256-byte aligned.  With H W = n pixels, in floats:
 *   with_grad = 1: the 13 ReLU outputs of x (270 n) + the 5 taps of y (122 n) + two ping-pong buffers of 64 n for y (they carry the
 *     gradient in backward) + the pooled x (16 n) + the head's gradient of one level (64 n) = 600 n floats: 1.54 GB at 800 x 800.
 *   with_grad = 0: two ping-pong buffers per image, 256 n floats: 0.66 GB at 800 x 800; the head runs level by level.
 *   Both: 5 x 1024 partial rows of 16 bytes.  The workspace of a with_grad forward must reach the backward unchanged.
 * mrgs_lpips_forward: terms[6] (device) = the five level terms and their sum.  mrgs_lpips_backward: g_total = device scalar, the upstream
 * gradient of terms[5]; g_x [3,H,W] is written in full (d terms[5] / d x times g_total); y gets none.  May be called again on the same
 * workspace: it changes only the gradient buffers.
 * mrgs_lpips_ws_offsets: byte offsets inside a with_grad workspace of the 13 stored ReLU outputs of x, then of the 5 taps of y (tests).
 * MRGS_E_BAD_ARG before any launch: wrong struct_size, H or W < 16 (the last stage would be empty) or H W > 2^24, with_grad other than
 * 0 / 1 (backward: other than 1), a NULL pointer, a blob or workspace not 256-byte aligned, ws_bytes too small. */
typedef struct MrgsLpipsConfig {
    uint32_t struct_size;           /* = sizeof(MrgsLpipsConfig) */
    int32_t H, W;
    float in_scale, in_offset;
    int32_t with_grad;
} MrgsLpipsConfig;
size_t mrgs_lpips_weights_bytes(void);
int mrgs_lpips_pack_weights(const float* const* conv_w /*[13]*/, const float* const* conv_b /*[13]*/, const float* const* lin_w /*[5]*/,
                            void* blob, void* stream);
size_t mrgs_lpips_ws_bytes(int32_t H, int32_t W, int32_t with_grad);
int mrgs_lpips_ws_offsets(int32_t H, int32_t W, size_t* offsets /*[18]*/);
int mrgs_lpips_forward(const MrgsLpipsConfig* cfg, const void* blob, const float* x, const float* y, void* ws, size_t ws_bytes,
                       float* terms /*[6]*/, void* stream);
int mrgs_lpips_backward(const MrgsLpipsConfig* cfg, const void* blob, void* ws, const float* g_total, float* g_x, void* stream);
/* One convolution launch of the network on caller tensors (tests).  (Cin, Cout) is one of the eight pairs above and names the weights
 * w [Cout,Cin,3,3] (torch layout; packed into ws first, ws_bytes >= 36 Cin Cout).  backward = 0: in [n][H][W][Cin] -> out [n][H][W][Cout]
 * = conv + bias (bias nullable).  backward = 1: the data gradient, in [n][H][W][Cout] -> out [n][H][W][Cin], no bias.  Then, in this
 * order: + add (nullable, shaped as out), ReLU when relu = 1, 0 where gate <= 0 (nullable, shaped as out).  The 3-channel side is planes
 * [n][3][H][W] instead: the input of the forward 3-64 (mapped as the network's input when zscore = 1, as it stands when 0) and the output
 * of the backward 64-3 (times in_scale / scale_c when zscore = 1); these two launches take no add and no gate.  n_images 1 or 2; any H, W
 * >= 1.  MRGS_E_BAD_ARG: wrong struct_size, an unserved pair, NULL in / w / out / ws, pointers not 16-byte aligned, a short ws. */
typedef struct MrgsLpipsConvConfig {
    uint32_t struct_size;           /* = sizeof(MrgsLpipsConvConfig) */
    int32_t H, W, Cin, Cout, n_images, backward, relu, zscore;
    float in_scale, in_offset;
} MrgsLpipsConvConfig;
int mrgs_lpips_debug_conv(const MrgsLpipsConvConfig* cfg, const float* in, const float* w, const float* bias, const float* add,
                          const float* gate, float* out, void* ws, size_t ws_bytes, void* stream);
/* The 2 x 2 maximum on a [H][W][C] (C a multiple of 4, H, W >= 1).  g_pooled NULL: out [H/2][W/2][C] = the maxima.  Otherwise out
 * [H][W][C] = g_pooled's entry at the window's FIRST maximum in row-major order (as torch), 0 elsewhere and in a last odd row or column. */
int mrgs_lpips_debug_pool(int32_t H, int32_t W, int32_t C, const float* a, const float* g_pooled, float* out, void* stream);
/* The head of one level alone: fx, fy [P][C] (C in {64, 128, 256, 512}), w [C]; ws = 1024 rows of 16 bytes.  term (device scalar) = the
 * level term; with g (device scalar) and g_fx [P][C] also its gradient with respect to fx times g. */
int mrgs_lpips_debug_head(int64_t P, int32_t C, const float* fx, const float* fy, const float* w, void* ws, size_t ws_bytes, float* term,
                          const float* g, float* g_fx, void* stream);

/* ---- evaluation of one rendered view (eval.py:23-102; evaluate_psnr / training_report, train_refreal.py:1656-1735) --------------------
 * mrgs_eval_metrics: image, gt [3,H,W] fp32 planes (a [4,H,W] ground truth passes its first three), both clamped to [0, 1] AS THEY ARE
 * READ (eval.py:44-46; no clamped copy is written).  Forward only, two launches, no host read.  out (device, 8 floats at any 4-byte aligned
 * address, e.g. row idx of an [n_views,8] table):
 *   [0] psnr_image    20 log10(1 / sqrt(mse over all 3 H W values))      utils/image_utils.py:20-23 on the [1,3,H,W] tensors of eval.py:51
 *   [1] ssim          utils/loss_utils.py:83-119: 11x11 window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over everything
 *   [2] l1            mean |image - gt|
 *   [3] psnr_channels mean over the channels of the per-channel psnr: psnr(image, gt).mean() on [3,H,W] tensors (train_refreal.py:1704,
 *                     :1730), the convention of out_terms[6] of mrgs_loss_forward
 *   [4..6] mse per channel    [7] 0
 * A zero mse gives +inf as the reference does.  Sums have a fixed order: two calls give the same bits.  ws: mrgs_eval_metrics_ws_bytes
 * (the per-workgroup partials, 48 bytes per 32x32 tile; 16-byte aligned).
 * MRGS_E_BAD_ARG before any HIP call: wrong struct_size, H or W <= 0, flags != 0, a NULL or misaligned pointer; MRGS_E_WORKSPACE for a
 * short ws; MRGS_E_UNSUPPORTED for H > 65535 * 32. */
typedef struct MrgsEvalConfig {
    uint32_t struct_size;           /* = sizeof(MrgsEvalConfig) */
    int32_t H, W;
    uint32_t flags;                 /* 0 */
} MrgsEvalConfig;
size_t mrgs_eval_metrics_ws_bytes(int32_t H, int32_t W);
int mrgs_eval_metrics(const MrgsEvalConfig* cfg, const float* image, const float* gt, void* ws, size_t ws_bytes, float* out /*[8]*/,
                      void* stream);
/* mrgs_export_rgb8: 1..MRGS_EXPORT_MAX_MAPS maps of one view, each [1,H,W] or [3,H,W] fp32 planes, to out uint8 [n_maps,H,W,3]
 * (pixel-interleaved, what a PNG row is; 4-byte aligned); a one-channel map is replicated to three bytes (eval.py:63-64).  Modes:
 *   UNIT    byte = trunc(clamp(x * 255 + 0.5, 0, 255)), the product and the sum rounded separately: torchvision.utils.save_image's
 *           mul(255).add_(0.5).clamp_(0, 255).to(uint8)
 *   NORMAL  the same after x * 0.5 + 0.5 (two roundings again; eval.py:56)
 *   DEPTH   visualize_depth (utils/image_utils.py:73-80) in fp32 and in its order: level = trunc(clip(((d - min) / (1e-20f + max - min))
 *           * 255, 0, 255)) with min / max over the map (reduced on the device, NaN skipped), the division correctly rounded; the three
 *           bytes are row `level` of the table mrgs_eval_jet_table returns (256 x 3, RGB).  One channel only.
 * The table is THIS LIBRARY'S OWN jet -- at v = level / 255 in double r = clamp(1.5 - |4 v - 3|, 0, 1), g = clamp(1.5 - |4 v - 2|, 0, 1),
 * b = clamp(1.5 - |4 v - 1|, 0, 1), byte = floor(255 c + 0.5) -- parity with cv2's COLORMAP_JET table unpinned; the level is what follows the
 * reference's statement.
 * NaN gives byte 0 in UNIT / NORMAL and level 0 in DEPTH (the reference's cast is undefined there).
 * At most two launches (one when no map is DEPTH), no host read.  ws: mrgs_export_ws_bytes(), needed (8-byte aligned) only with a DEPTH map.
 * MRGS_E_BAD_ARG before any HIP call: wrong struct_size, H or W <= 0, flags != 0, n_maps outside 1..MRGS_EXPORT_MAX_MAPS, a NULL or
 * misaligned pointer, channels other than 1 / 3, an unknown mode, DEPTH with three channels; MRGS_E_WORKSPACE for a short ws. */
#define MRGS_EXPORT_MAX_MAPS 16
enum { MRGS_EXPORT_UNIT = 0, MRGS_EXPORT_NORMAL = 1, MRGS_EXPORT_DEPTH = 2 };
typedef struct MrgsExportMap {
    const float* data;              /* [channels,H,W] */
    int32_t channels, mode;
} MrgsExportMap;
typedef struct MrgsExportConfig {
    uint32_t struct_size;           /* = sizeof(MrgsExportConfig) */
    int32_t H, W, n_maps;
    uint32_t flags;                 /* 0 */
} MrgsExportConfig;
size_t mrgs_export_ws_bytes(void);
int mrgs_export_rgb8(const MrgsExportConfig* cfg, const MrgsExportMap* maps, void* ws, size_t ws_bytes, uint8_t* out, void* stream);
int mrgs_eval_jet_table(uint8_t* table768 /*host, [256][3]*/);

/* ---- the training contact sheet (save_training_vis, train_refreal.py:1513-1620; the same in train_refnerf.py and train_glossy.py) ------
 * mrgs_sheet_rgb8: 1..MRGS_SHEET_MAX_CELLS cells of one H x W, laid out as torchvision.utils.make_grid(nrow, padding, pad_value 0) lays
 * them out, resampled as F.interpolate's default (legacy) nearest does, to out uint8 [Ho,Wo,3] (pixel-interleaved, 4-byte aligned) -- every
 * byte computed from the cells' own planes: no stack, no grid and no resampled tensor exist.
 *   grid      xmaps = min(nrow, n_cells), ymaps = ceil(n_cells / xmaps), Hg = (H + padding) ymaps + padding, Wg = (W + padding) xmaps +
 *             padding; cell k has its corner at ((k / xmaps) (H + padding) + padding, (k % xmaps) (W + padding) + padding); the borders and
 *             the unused places of the last row are 0.  n_cells = 1: the image itself, Hg = H, Wg = W (make_grid's early return).
 *   resample  source index = min((int)floorf(dst * scale), in - 1) per axis, one fp32 multiply; scale_y = (float)Hg / (float)Ho and
 *             scale_x = (float)Wg / (float)Wo are computed by the caller in fp32 (what F.interpolate computes).  Ho = Hg, Wo = Wg with
 *             scales 1 is the identity.
 * Cell modes (fp32, every product and sum rounded on its own; `UNIT rule` and the jet table are mrgs_export_rgb8's):
 *   UNIT         [1|3,H,W]: the UNIT rule; one channel is replicated
 *   ABSDIFF      data, data2 [3,H,W]: |data - data2|, then the UNIT rule                                  (error_map, :1518)
 *   NORMAL_VIEW  [3,H,W]: y = rot x per pixel, y_i = (rot[3i] x_0 + rot[3i+1] x_1) + rot[3i+2] x_2, channels permuted to [2,1,0],
 *                0.5 y + 0.5, then the UNIT rule                                                          (a(x), :1521-1524)
 *   DEPTH        [1,H,W]: mrgs_export_rgb8's DEPTH                                                        (visualize_depth)
 *   LEVEL        [1,H,W]: level = trunc(clip(x * 255, 0, 255)), then jet                                  (visualize_depth(norm=False))
 *   DEPTH2       [1,H,W]: std = the population standard deviation of the map, accumulated in double on the device from the fp32 values and
 *                rounded once to fp32; x clipped to [0, 6.f * std]; then DEPTH on the clipped map        (visualize_depth2,
 *                utils/image_utils.py:83-93).  A map with an infinite value has no std: level 0 throughout.
 *   MASK         [H W] fp32 (elem F32) or bytes (elem U8: uint8 / bool): level = trunc(clip(float(m) * 255, 0, 255)), then jet
 *                (visualize_d_mask; the reference's cast of a value outside [0, 255] is undefined, here it clamps)
 * NaN gives byte 0 / level 0 and is skipped by the statistics (minimum, maximum, std).
 * At most two launches (one when no cell is DEPTH / DEPTH2), no host read, no allocation.  ws: mrgs_sheet_ws_bytes(), needed (16-byte
 * aligned) only with a DEPTH / DEPTH2 cell.
 * MRGS_E_BAD_ARG before any HIP call: wrong struct_size, H, W, Ho or Wo <= 0, n_cells outside 1..MRGS_SHEET_MAX_CELLS, nrow < 1,
 * padding < 0, flags != 0, a scale that is not positive and finite, a NULL or misaligned pointer, an unknown mode or element type (U8 with
 * MASK only), channels that do not fit the mode (UNIT 1 or 3; ABSDIFF, NORMAL_VIEW 3; the others 1), ABSDIFF without data2, Ho Wo 3 or a
 * grid dimension beyond int32; MRGS_E_WORKSPACE for a short ws. */
#define MRGS_SHEET_MAX_CELLS 32
enum { MRGS_SHEET_UNIT = 0, MRGS_SHEET_ABSDIFF = 1, MRGS_SHEET_NORMAL_VIEW = 2, MRGS_SHEET_DEPTH = 3, MRGS_SHEET_LEVEL = 4,
       MRGS_SHEET_DEPTH2 = 5, MRGS_SHEET_MASK = 6 };
enum { MRGS_SHEET_ELEM_F32 = 0, MRGS_SHEET_ELEM_U8 = 1 };
typedef struct MrgsSheetCell {
    const void* data;               /* [channels,H,W] fp32; MASK: [H W] fp32 or bytes */
    const void* data2;              /* ABSDIFF: the second image; otherwise not read */
    int32_t channels, mode;
    int32_t elem;                   /* MRGS_SHEET_ELEM_*: the element type of a MASK cell; F32 for every other mode */
    int32_t reserved;               /* 0 */
} MrgsSheetCell;
typedef struct MrgsSheetConfig {
    uint32_t struct_size;           /* = sizeof(MrgsSheetConfig) */
    int32_t H, W, n_cells, nrow, padding, Ho, Wo;
    float scale_y, scale_x;         /* (float)Hg / (float)Ho, (float)Wg / (float)Wo */
    float rot[9];                   /* row-major 3x3 of NORMAL_VIEW (viewpoint_cam.R.T); not read without such a cell */
    uint32_t flags;                 /* 0 */
} MrgsSheetConfig;
size_t mrgs_sheet_ws_bytes(void);
int mrgs_sheet_rgb8(const MrgsSheetConfig* cfg, const MrgsSheetCell* cells, void* ws, size_t ws_bytes, uint8_t* out /*[Ho,Wo,3]*/,
                    void* stream);

/* ---- the dataset side of a view: 8-bit planes on the device (scene/dataset_readers.py, utils/camera_utils.py, utils/general_utils.py) ----
 * mrgs_image_resize_u8: `pil_image.resize((out_w, out_h))` of PILtoTorch (general_utils.py:21-27), i.e. Pillow's BICUBIC on 8-bit
 * channels, bit for bit.  src: `channels` (1..4) byte channels of an in_h x in_w image, element (c, y, x) at byte c stride_c + y stride_y +
 * x stride_x (a pixel-interleaved [H,W,C] image is stride (1, W C, C), planes are (H W, W, 1)); dst: planes [channels][out_h][out_w].
 * Channels are independent (RGBA is four L images, no premultiplication).  Per resized axis the caller passes the coefficient table Pillow
 * computes, as DEVICE arrays: bounds [out][2] int32 = (first source index, tap count n), kk [out][ksize] int32 = the normalised Keys
 * (a = -0.5) weights times 2^22, rounded half away from zero.  A pass writes clip8((2^21 + sum_{t<n} kk[t] * pixel[first + t]) >> 22),
 * arithmetic shift; the horizontal pass runs first over every source row into an 8-bit intermediate, then the vertical pass.  An axis whose
 * size does not change has no pass and needs no table (NULL); equal sizes are a copy into planes.  The tables are READ AS GIVEN: first >= 0
 * and first + n <= the source extent are the caller's contract (materialrefgs_amd/viewstore.py: resize_table builds them).
 * ws: mrgs_image_resize_ws_bytes bytes (channels in_h out_w when both axes change, else 0).  At most two launches, no host read.
 * MRGS_E_BAD_ARG before any HIP call: wrong struct_size, flags != 0, channels outside 1..4, a size outside 1..2^24, a stride_y / stride_x
 * <= 0 or stride_c < 0, NULL src / dst, a missing table or ksize < 1 for an axis that changes, NULL ws when one is needed;
 * MRGS_E_WORKSPACE for a short ws. */
typedef struct MrgsResizeConfig {
    uint32_t struct_size;           /* = sizeof(MrgsResizeConfig) */
    int32_t channels, in_h, in_w, out_h, out_w;
    int32_t ksize_x, ksize_y;       /* row length of kk_x / kk_y */
    uint32_t flags;                 /* 0 */
    int64_t stride_c, stride_y, stride_x;
} MrgsResizeConfig;
size_t mrgs_image_resize_ws_bytes(int32_t channels, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w);
int mrgs_image_resize_u8(const MrgsResizeConfig* cfg, const uint8_t* src, const int32_t* bounds_x, const int32_t* kk_x,
                         const int32_t* bounds_y, const int32_t* kk_y, void* ws, size_t ws_bytes, uint8_t* dst, void* stream);
/* mrgs_image_composite_u8: readCamerasFromTransforms' compositing onto a constant background (dataset_readers.py:276-282).  rgba
 * [n_pixels][4] bytes (4-byte aligned), table [256][256] device bytes indexed [colour][alpha] -- the host evaluates the reference's float64
 * expression and its wrapping cast once per (colour, alpha) pair and background -- dst planes [3][n_pixels].  One launch.
 * MRGS_E_BAD_ARG: n_pixels < 0 or >= 2^36, a NULL pointer or a misaligned rgba with n_pixels > 0; n_pixels = 0 returns MRGS_OK. */
int mrgs_image_composite_u8(int64_t n_pixels, const uint8_t* rgba, const uint8_t* table, uint8_t* dst, void* stream);
/* mrgs_view_decode: one launch turns the byte planes of a view into the fp32 tensors the losses read.  Every output may be NULL; an
 * output that is not NULL needs its input.
 *   gt [3,H,W]         = rgb [3,H,W] / 255.0f, IEEE division: torch's `uint8_tensor / 255.0`
 *   alpha_out [1,H,W]  = alpha [H,W] / 255.0f
 *   grey [1,Hg,Wg]     = (0.299f r + 0.587f g) + 0.114f b on r, g, b = grey_rgb [3,Hg,Wg] / 255.0f, every product and sum rounded on its
 *                        own (utils/camera_utils.py:37); grey_rgb is rgb itself when the grey image has the image's size
 *   normal_out [H W,3] = normal_table[normal [H,W,3]]; the table (256 device floats) is float32((n / 255.) * 2. - 1) from float64
 *   mask_out [H W,1]   = mask [H,W] > 128 ? 1 : 0        (train_refnerf.py:124)
 *   score_out [1,H,W]  = score [H,W] > 128 as bool bytes (train_refnerf.py:193)
 * MRGS_E_BAD_ARG before any HIP call: wrong struct_size, flags != 0, H or W outside 1..2^24 (Hg, Wg with grey), no output at all, an output
 * without its input, a float pointer that is not 4-byte aligned. */
typedef struct MrgsViewDecode {
    uint64_t struct_size;           /* = sizeof(MrgsViewDecode) */
    int32_t H, W, Hg, Wg;
    const uint8_t* rgb;
    const uint8_t* alpha;
    const uint8_t* grey_rgb;
    const uint8_t* normal;
    const uint8_t* mask;
    const uint8_t* score;
    const float* normal_table;
    float* gt;
    float* alpha_out;
    float* grey;
    float* normal_out;
    float* mask_out;
    uint8_t* score_out;
    uint64_t flags;                 /* 0 */
} MrgsViewDecode;
int mrgs_view_decode(const MrgsViewDecode* view, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRGS_H_INCLUDED */
