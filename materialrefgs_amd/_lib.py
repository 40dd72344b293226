"""ctypes binding of libmrgs.so (the C ABI declared in include/mrgs.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing the rasterizer
raises.  torch is imported first so that libmrgs.so binds to the HIP runtime torch already loaded
(same SONAME libamdhip64.so.7) and therefore shares its devices, streams and allocations.
"""
import ctypes
import os
import subprocess

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# MRGS_LIB: developer override to load another build of the same library (kernel experiments); never a fallback
LIB_PATH = os.environ.get("MRGS_LIB") or os.path.join(_CSRC, "libmrgs.so")

c_int32, c_int64, c_float, c_void_p, c_size_t = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t


class _Sized(ctypes.Structure):
    """Structs whose first field is `struct_size` (include/mrgs.h): filled in here, so positional arguments start at the second field."""

    def __init__(self, *args, **kw):
        super().__init__(ctypes.sizeof(type(self)), *args, **kw)


class MrgsRasterConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("P", c_int32), ("S", c_int32), ("D", c_int32), ("M", c_int32), ("H", c_int32), ("W", c_int32),
                ("tanfovx", c_float), ("tanfovy", c_float), ("scale_modifier", c_float), ("prefiltered", c_int32),
                ("debug", c_int32)]


class MrgsRasterInputs(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, c_void_p) for n in ("bg", "means3D", "shs", "colors_precomp", "features", "opacities", "scales",
                                        "rotations", "transMat_precomp", "viewmatrix", "projmatrix", "campos", "work_hint", "shs_rest",
                                        "bwd_grad_ws")] + [("hint_flags", ctypes.c_uint32), ("features_live", ctypes.c_uint32)]


MRGS_HINT_REUSE_ORDER = 1
MRGS_HINT_VISIBLE_BYTES = 2


class MrgsRasterGrads(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, c_void_p) for n in ("dL_dmeans2D", "dL_dcolors", "dL_dfeatures", "dL_dopacity", "dL_dmeans3D",
                                        "dL_dtransMat", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dsh_rest",
                                        "glue_params", "glue_grads")]     # ABI 10: the glue epilogue (pointers to MrgsSurfelParams / MrgsSurfelGrads)


MRGS_MAX_MIPS = 8


class MrgsEnvMips(ctypes.Structure):
    _fields_ = [("n_levels", c_int32), ("res", c_int32 * MRGS_MAX_MIPS), ("tex", c_void_p * MRGS_MAX_MIPS),
                ("grad", c_void_p * MRGS_MAX_MIPS), ("grad_copies", c_int32 * MRGS_MAX_MIPS), ("min_roughness", c_float), ("max_roughness", c_float)]


class MrgsStridedMap(ctypes.Structure):
    _fields_ = [("ptr", c_void_p), ("stride_h", c_int64), ("stride_w", c_int64), ("stride_c", c_int64)]


class MrgsShadeFrame(ctypes.Structure):
    _fields_ = [("H", c_int32), ("W", c_int32), ("Kinv", c_float * 9), ("R", c_void_p), ("T", c_void_p),
                ("albedo", MrgsStridedMap), ("normal", MrgsStridedMap), ("alpha", MrgsStridedMap), ("refl", MrgsStridedMap),
                ("roughness", MrgsStridedMap), ("lut", c_void_p), ("lut_res", c_int32)]


class MrgsBounceConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_rays", c_int64), ("n_vertices", c_int64),
                ("n_triangles", c_int64), ("base_res", c_int32), ("lut_res", c_int32)]


class MrgsRasterTicket(ctypes.Structure):
    _fields_ = [("device", c_int32), ("slot", c_int32), ("seq", ctypes.c_uint64), ("capacity_pairs", c_int64)]


class MrgsSpmvDesc(ctypes.Structure):
    _fields_ = [("nrows", c_int32), ("lanes_per_row", c_int32), ("col_bytes", c_int32), ("val_bytes", c_int32), ("row_ptr", c_void_p),
                ("col", c_void_p), ("val", c_void_p), ("row_scale", c_void_p), ("x", c_void_p), ("y", c_void_p),
                ("image_rows", c_void_p), ("pre_scale", c_void_p), ("tile_ptr", c_void_p), ("panel_ptr", c_void_p), ("panel_src", c_void_p),
                ("res", c_int32), ("n_tiles", c_int32), ("max_panel", c_int32), ("reserved", c_int32)]


class MrgsSurfelParams(ctypes.Structure):
    _fields_ = [("P", c_int32)] + [(n, c_void_p) for n in ("xyz", "scaling_raw", "rotation_raw", "opacity_raw", "refl_raw", "rough_raw",
                                                             "ori_color_raw", "indirect_dc", "indirect_rest", "campos", "viewmatrix")]


class MrgsSurfelGrads(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("d_xyz", "d_scaling", "d_rotation", "d_opacity", "d_refl", "d_rough", "d_ori_color",
                                        "d_indirect_dc", "d_indirect_rest")]


class MrgsVolumeParams(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("P", c_int32)] + \
               [(n, c_void_p) for n in ("xyz", "scaling_raw", "rotation_raw", "opacity_raw", "refl_raw", "rough_raw", "ori_color_raw", "campos",
                                        "rays_o", "lut", "viewmatrix")] + [("lut_res", c_int32), ("reserved", c_int32)]


class MrgsVolumeGrads(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, c_void_p) for n in ("d_xyz", "d_scaling", "d_rotation", "d_opacity", "d_refl", "d_rough",
                                                                             "d_ori_color")]


class MrgsMapsFrame(ctypes.Structure):
    _fields_ = [("H", c_int32), ("W", c_int32), ("view_rot", c_float * 9), ("ray_matrix", c_float * 9), ("ray_origin", c_float * 3),
                ("depth_ratio", c_float), ("pgsr_fx", c_float), ("pgsr_fy", c_float), ("rend_distance", c_void_p), ("g_rend_distance", c_void_p)]


class MrgsLossConfig(ctypes.Structure):
    _fields_ = [("H", c_int32), ("W", c_int32), ("C", c_int32), ("lambda_dssim", c_float), ("lambda_normal", c_float),
                ("lambda_dist", c_float)]


class MrgsPriorConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("flags", ctypes.c_uint32)]


MRGS_SMOOTH_MAX_ITEMS = 4


class MrgsSmoothConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("flags", ctypes.c_uint32)]


class MrgsSmoothItem(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("mask", c_void_p), ("g_data", c_void_p), ("C", c_int32), ("edge_aware", c_int32)]


MRGS_WARP_GEO, MRGS_WARP_MATERIAL, MRGS_WARP_METALLIC, MRGS_WARP_ROUGHNESS = 1, 2, 4, 8


class MrgsWarpConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("sample_num", c_int32), ("patch_half", c_int32),
                ("n_given", c_int32), ("flags", ctypes.c_uint32), ("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32)] + \
               [(n, c_float) for n in ("fx_v", "fy_v", "cx_v", "cy_v", "fx_n", "fy_n", "cx_n", "cy_n", "pixel_noise_th", "geo_weight",
                                       "base_weight", "metallic_weight", "roughness_weight")]


class MrgsWarpMaps(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("depth_v", "depth_n", "normal_v", "distance_v", "base_v", "metal_v", "rough_v", "base_n", "metal_n",
                                        "rough_n", "fg_v", "keep_v", "cam_v", "cam_n")]


class MrgsRefScoreConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("patch_half", c_int32), ("n_neighbours", c_int32)] + \
               [(n, c_float) for n in ("fx_v", "fy_v", "cx_v", "cy_v", "pixel_noise_th")]


class MrgsRefScoreNeighbour(ctypes.Structure):
    _fields_ = [("depth", c_void_p), ("image", c_void_p), ("cam", c_float * 28), ("fx", c_float), ("fy", c_float), ("cx", c_float),
                ("cy", c_float)]


class MrgsAdamTensor(ctypes.Structure):
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("numel", c_int64),
                ("lr", c_float), ("step", c_int32)]


MRGS_ADAM_ROWS_MAX_MASKS = 4


class MrgsAdamRowsTensor(ctypes.Structure):
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("numel", c_int64),
                ("row_floats", c_int32), ("lr", c_float), ("step", c_int32), ("reserved", c_int32)]


class MrgsCompactTensor(ctypes.Structure):
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("row_floats", c_int32)]


MRGS_DENSIFY_COPY, MRGS_DENSIFY_MOMENT, MRGS_DENSIFY_XYZ, MRGS_DENSIFY_SCALING = 0, 1, 2, 3


class MrgsDensifyConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("N", c_int32), ("P", c_int64), ("max_grad", c_float), ("min_opacity", c_float),
                ("percent_dense_extent", c_float), ("world_size_limit", c_float), ("xyz_raw", c_void_p), ("scaling_raw", c_void_p),
                ("rotation_raw", c_void_p)]


class MrgsDensifyTensor(ctypes.Structure):
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("row_floats", c_int32), ("role", c_int32)]


MRGS_ENV_DENSIFY_SCREEN, MRGS_ENV_DENSIFY_SPLIT_SCREEN, MRGS_ENV_DENSIFY_COUNTS = 1, 2, 40


class MrgsEnvDensifyConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("P", c_int64), ("n_after", c_int64), ("max_grad", c_float),
                ("min_opacity", c_float), ("percent_dense_extent", c_float), ("world_size_limit", c_float), ("max_screen_size", c_float),
                ("reserved", c_float), ("xyz_raw", c_void_p), ("scaling_raw", c_void_p), ("rotation_raw", c_void_p)]


MRGS_TSDF_CONTRACTED, MRGS_TSDF_PLAIN, MRGS_TSDF_POINTS = 0, 1, 2


class MrgsTsdfView(ctypes.Structure):
    _fields_ = [("proj", c_float * 16), ("depth", c_void_p), ("H", c_int32), ("W", c_int32)]


class MrgsTsdfConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("mode", c_int32), ("n0", c_int32), ("n1", c_int32), ("n2", c_int32), ("n_views", c_int32),
                ("n_points", c_int64), ("origin", c_float * 3), ("spacing", c_float * 3), ("center", c_float * 3), ("radius", c_float),
                ("trunc", c_float), ("depth_trunc", c_float), ("points", c_void_p)]


class MrgsAttrView(ctypes.Structure):
    _fields_ = [("proj", c_float * 16), ("depth", c_void_p), ("attr", c_void_p), ("H", c_int32), ("W", c_int32)]


class MrgsVertexFuseConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_views", c_int32), ("n_points", c_int64), ("channels", c_int32), ("w0", c_int32),
                ("trunc", c_float), ("depth_trunc", c_float)]


class MrgsMeshConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n0", c_int32), ("n1", c_int32), ("n2", c_int32), ("slab_planes", c_int32),
                ("contracted", c_int32), ("level", c_float), ("origin", c_float * 3), ("spacing", c_float * 3), ("center", c_float * 3),
                ("radius", c_float)]


MRGS_RESET_MAX_ITEMS = 8
(MRGS_RESET_CAP, MRGS_RESET_FLOOR, MRGS_RESET_LIFT, MRGS_RESET_CONST, MRGS_RESET_FILL, MRGS_RESET_JITTER, MRGS_RESET_JITTER_CONST,
 MRGS_RESET_ENLARGE) = range(8)
MRGS_RESET_KEEP_EXCLUSIVE, MRGS_RESET_KEEP_REFL_ABOVE, MRGS_RESET_KEEP_REFL_BELOW, MRGS_RESET_KEEP_ROUGH_ABOVE = 1, 2, 4, 8


class MrgsResetItem(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("src", "dst", "exp_avg_dst", "exp_avg_sq_dst", "noise")] + \
               [(n, c_int32) for n in ("width", "rule", "keep", "reserved")] + [("a", ctypes.c_double), ("b", ctypes.c_double)]


class MrgsResetConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("P", c_int64), ("refl_raw", c_void_p), ("rough_raw", c_void_p), ("exclusive", c_void_p),
                ("refl_thr", c_float), ("rough_thr", c_float), ("seed", ctypes.c_uint64)]


class MrgsLpipsConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("in_scale", c_float), ("in_offset", c_float),
                ("with_grad", c_int32)]


class MrgsLpipsConvConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, c_int32) for n in ("H", "W", "Cin", "Cout", "n_images", "backward", "relu", "zscore")] + \
               [("in_scale", c_float), ("in_offset", c_float)]


class MrgsEvalConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("flags", ctypes.c_uint32)]


MRGS_EXPORT_MAX_MAPS = 16
MRGS_EXPORT_UNIT, MRGS_EXPORT_NORMAL, MRGS_EXPORT_DEPTH = 0, 1, 2


class MrgsExportMap(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("channels", c_int32), ("mode", c_int32)]


class MrgsExportConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32), ("H", c_int32), ("W", c_int32), ("n_maps", c_int32), ("flags", ctypes.c_uint32)]


MRGS_SHEET_MAX_CELLS = 32
(MRGS_SHEET_UNIT, MRGS_SHEET_ABSDIFF, MRGS_SHEET_NORMAL_VIEW, MRGS_SHEET_DEPTH, MRGS_SHEET_LEVEL, MRGS_SHEET_DEPTH2,
 MRGS_SHEET_MASK) = range(7)
MRGS_SHEET_ELEM_F32, MRGS_SHEET_ELEM_U8 = 0, 1


class MrgsSheetCell(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("data2", c_void_p), ("channels", c_int32), ("mode", c_int32), ("elem", c_int32), ("reserved", c_int32)]


class MrgsSheetConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, c_int32) for n in ("H", "W", "n_cells", "nrow", "padding", "Ho", "Wo")] + \
               [("scale_y", c_float), ("scale_x", c_float), ("rot", c_float * 9), ("flags", ctypes.c_uint32)]


class MrgsResizeConfig(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, c_int32) for n in ("channels", "in_h", "in_w", "out_h", "out_w", "ksize_x", "ksize_y")] + \
               [("flags", ctypes.c_uint32), ("stride_c", c_int64), ("stride_y", c_int64), ("stride_x", c_int64)]


class MrgsViewDecode(_Sized):
    _fields_ = [("struct_size", ctypes.c_uint64)] + [(n, c_int32) for n in ("H", "W", "Hg", "Wg")] + \
               [(n, c_void_p) for n in ("rgb", "alpha", "grey_rgb", "normal", "mask", "score", "normal_table", "gt", "alpha_out", "grey",
                                        "normal_out", "mask_out", "score_out")] + [("flags", ctypes.c_uint64)]


class MrgsDepthView(ctypes.Structure):
    _fields_ = [("depth", c_void_p), ("R", c_float * 9), ("T", c_float * 3), ("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float)]


class MrgsKernelTimes(ctypes.Structure):
    _fields_ = [(n, c_float) for n in ("preprocess_ms", "sort_ms", "duplicate_ms", "render_fwd_ms", "render_bwd_ms",
                                       "preprocess_bwd_ms")]


# every symbol include/mrgs.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mrgs_geom_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "mrgs_img_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_binning_bytes": (c_size_t, [c_int64]),
    "mrgs_work_hint_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_grad_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_rasterize_forward_geom": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p,
                                                   c_size_t, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "mrgs_rasterize_forward_render": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p,
                                                     c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_rasterize_forward": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p, c_size_t,
                                              c_void_p, c_size_t, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              ctypes.POINTER(c_int64), c_void_p]),
    "mrgs_rasterize_forward_begin": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p, c_size_t,
                                                    c_void_p, c_size_t, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    ctypes.POINTER(MrgsRasterTicket), c_void_p]),
    "mrgs_rasterize_forward_finish": (ctypes.c_int, [ctypes.POINTER(MrgsRasterTicket), ctypes.POINTER(c_int64)]),
    "mrgs_rasterize_backward": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                               ctypes.POINTER(MrgsRasterGrads), c_void_p]),
    "mrgs_rasterize_backward_blend": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_rasterize_backward_finish": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), ctypes.POINTER(MrgsRasterInputs), c_void_p, c_void_p,
                                                      c_void_p, ctypes.POINTER(MrgsRasterGrads), c_void_p]),
    "mrgs_surfel_features_forward": (ctypes.c_int, [ctypes.POINTER(MrgsSurfelParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_surfel_features_backward": (ctypes.c_int, [ctypes.POINTER(MrgsSurfelParams), c_void_p, c_void_p, c_void_p, c_void_p,
                                                     ctypes.POINTER(MrgsSurfelGrads), c_void_p, c_void_p]),
    "mrgs_surfel_maps_forward": (ctypes.c_int, [ctypes.POINTER(MrgsMapsFrame), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p]),
    "mrgs_surfel_maps_backward": (ctypes.c_int, [ctypes.POINTER(MrgsMapsFrame), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_surfel_composite_forward": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_void_p]),
    "mrgs_surfel_composite_backward": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mrgs_cubemap_filter_count": (ctypes.c_int, [c_int32, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "mrgs_cubemap_filter_fill": (ctypes.c_int, [c_int32, c_int32, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_csr_spmv3": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "mrgs_csr_spmv3_batched": (ctypes.c_int, [ctypes.POINTER(MrgsSpmvDesc), c_int32, c_void_p]),
    "mrgs_cube_symmetry_rows": (ctypes.c_int, [c_int32, c_void_p]),
    "mrgs_cubemap_mip_chain_forward": (ctypes.c_int, [c_int32, c_int32, c_void_p, ctypes.POINTER(c_void_p), c_void_p]),
    "mrgs_cubemap_mip_chain_backward": (ctypes.c_int, [c_int32, c_int32, ctypes.POINTER(c_void_p), c_void_p]),
    "mrgs_cubemap_mip_forward": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p]),
    "mrgs_cubemap_mip_backward": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p]),
    "mrgs_surfel_feature_grads": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 11),
    "mrgs_loss_ws_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "mrgs_loss_forward": (ctypes.c_int, [ctypes.POINTER(MrgsLossConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "mrgs_loss_backward": (ctypes.c_int, [ctypes.POINTER(MrgsLossConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_prior_ws_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_prior_terms_forward": (ctypes.c_int, [ctypes.POINTER(MrgsPriorConfig), ctypes.POINTER(c_float)] + [c_void_p] * 10 + [c_size_t, c_void_p,
                                                                                                                          c_void_p]),
    "mrgs_prior_terms_backward": (ctypes.c_int, [ctypes.POINTER(MrgsPriorConfig), ctypes.POINTER(c_float)] + [c_void_p] * 10 +
                                  [ctypes.POINTER(c_void_p)] + [c_void_p] * 6),
    "mrgs_smooth_ws_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_smooth_terms_forward": (ctypes.c_int, [ctypes.POINTER(MrgsSmoothConfig), c_void_p, ctypes.POINTER(MrgsSmoothItem), c_int32, c_void_p,
                                                 c_size_t, c_void_p, c_void_p]),
    "mrgs_smooth_terms_backward": (ctypes.c_int, [ctypes.POINTER(MrgsSmoothConfig), c_void_p, ctypes.POINTER(MrgsSmoothItem), c_int32,
                                                  ctypes.POINTER(c_void_p), c_void_p]),
    "mrgs_warp_loss_ws_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "mrgs_warp_loss_forward": (ctypes.c_int, [ctypes.POINTER(MrgsWarpConfig), ctypes.POINTER(MrgsWarpMaps), c_void_p, c_void_p, c_size_t,
                                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_warp_loss_backward": (ctypes.c_int, [ctypes.POINTER(MrgsWarpConfig), ctypes.POINTER(MrgsWarpMaps)] + [c_void_p] * 12),
    "mrgs_warp_ncc_ws_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "mrgs_warp_ncc_forward": (ctypes.c_int, [ctypes.POINTER(MrgsWarpConfig), ctypes.POINTER(MrgsWarpMaps), c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_float] + [c_void_p] * 6),
    "mrgs_warp_ncc_backward": (ctypes.c_int, [ctypes.POINTER(MrgsWarpConfig), c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "mrgs_ref_score": (ctypes.c_int, [ctypes.POINTER(MrgsRefScoreConfig)] + [c_void_p] * 9),
    "mrgs_bvh_bytes": (c_size_t, [c_int64]),
    "mrgs_bvh_build": (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_size_t]),
    "mrgs_bvh_trace": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_bvh_visibility": (ctypes.c_int, [c_void_p, c_int64, c_int32, c_int32, ctypes.POINTER(c_float), c_void_p, c_void_p,
                                           ctypes.POINTER(MrgsStridedMap), ctypes.POINTER(MrgsStridedMap), c_void_p, c_void_p, c_void_p]),
    "mrgs_adam_step": (ctypes.c_int, [ctypes.POINTER(MrgsAdamTensor), c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_void_p]),
    "mrgs_adam_step_rows": (ctypes.c_int, [ctypes.POINTER(MrgsAdamRowsTensor), c_int32, c_int64, ctypes.POINTER(c_void_p), c_int32, c_int32,
                                           ctypes.c_double, ctypes.c_double, ctypes.c_double, c_void_p]),
    "mrgs_indirect_blend_forward": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, ctypes.POINTER(MrgsStridedMap),
                                                   ctypes.POINTER(MrgsStridedMap), c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_indirect_blend_backward": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, ctypes.POINTER(MrgsStridedMap),
                                                    ctypes.POINTER(MrgsStridedMap), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p]),
    "mrgs_cubemap_encode_forward": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int32, c_int32, c_void_p]),
    "mrgs_cubemap_encode_backward": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int32,
                                                    c_int32, c_void_p]),
    "mrgs_surfel_bvh_bytes": (c_size_t, [c_int64]),
    "mrgs_surfel_bvh_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_surfel_trace_state_floats": (c_size_t, [c_int64, c_int32]),
    "mrgs_surfel_trace_state_floats_norecord": (c_size_t, [c_int64, c_int32]),
    "mrgs_surfel_trace_state_layout": (ctypes.c_int, [c_int64, c_int32, ctypes.POINTER(c_size_t)]),
    "mrgs_mirror_rays_forward": (ctypes.c_int, [c_int32, c_int32, ctypes.POINTER(c_float), c_void_p, c_void_p, ctypes.POINTER(MrgsStridedMap), c_void_p,
                                                c_void_p, c_void_p, c_void_p]),
    "mrgs_mirror_rays_backward": (ctypes.c_int, [c_int32, c_int32, ctypes.POINTER(c_float), c_void_p, c_void_p, ctypes.POINTER(MrgsStridedMap), c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_mirror_rays_blended_forward": (ctypes.c_int, [c_int32, c_int32, ctypes.POINTER(c_float), c_void_p, c_void_p, ctypes.POINTER(MrgsStridedMap),
                                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_mirror_rays_blended_backward": (ctypes.c_int, [c_int32, c_int32, ctypes.POINTER(c_float), c_void_p, c_void_p, ctypes.POINTER(MrgsStridedMap),
                                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_traced_blend_forward": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "mrgs_traced_blend_backward": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64] + [c_void_p] * 5),
    "mrgs_surfel_trace_prep_raw_forward": (ctypes.c_int, [c_int64] + [c_void_p] * 6 + [c_int32] + [c_void_p] * 2 + [c_float] + [c_void_p] * 4),
    "mrgs_surfel_trace_prep_raw_backward": (ctypes.c_int, [c_int64] + [c_void_p] * 6 + [c_int32, c_void_p, c_float] + [c_void_p] * 10),
    "mrgs_surfel_trace_prep_forward": (ctypes.c_int, [c_int64] + [c_void_p] * 5 + [c_int32, c_int32] + [c_void_p] * 3 + [c_float] + [c_void_p] * 4),
    "mrgs_surfel_trace_prep_backward": (ctypes.c_int, [c_int64] + [c_void_p] * 4 + [c_int32, c_int32, c_void_p, c_float] + [c_void_p] * 10),
    "mrgs_surfel_bvh_build": (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "mrgs_surfel_trace_forward": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int32] + [c_void_p] * 4 + [ctypes.POINTER(c_float)] + [c_void_p] * 8 + [c_size_t, c_void_p]),
    "mrgs_surfel_trace_backward": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int32] + [c_void_p] * 4 + [ctypes.POINTER(c_float)] + [c_void_p] * 6 + [c_size_t] + [c_void_p] * 11),
    "mrgs_sh_grad_expand": (ctypes.c_int, [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "mrgs_sh_grad_expand_surfel": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p]),
    "mrgs_sh_grad_expand_surfel_rows": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                                       c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_compact_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_compact_count": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_compact_rows": (ctypes.c_int, [c_int64, c_void_p, c_void_p, ctypes.POINTER(MrgsCompactTensor), c_int32, c_void_p]),
    "mrgs_densify_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_densify_classify": (ctypes.c_int, [ctypes.POINTER(MrgsDensifyConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                             c_void_p, c_void_p]),
    "mrgs_densify_emit": (ctypes.c_int, [ctypes.POINTER(MrgsDensifyConfig), c_void_p, ctypes.POINTER(c_int64),
                                         ctypes.POINTER(MrgsDensifyTensor), c_int32, ctypes.c_uint64, c_void_p, c_void_p]),
    "mrgs_densify_stats": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_env_densify_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_env_densify_classify": (ctypes.c_int, [ctypes.POINTER(MrgsEnvDensifyConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_env_densify_emit": (ctypes.c_int, [ctypes.POINTER(MrgsEnvDensifyConfig), c_void_p, c_int64, ctypes.POINTER(MrgsDensifyTensor), c_int32,
                                             ctypes.c_uint64, c_void_p, c_void_p, c_void_p]),
    "mrgs_env_select_ws_bytes": (c_size_t, []),
    "mrgs_env_select": (ctypes.c_int, [c_int64, c_void_p, c_int64, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_env_densify_stats": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_tsdf_fuse": (ctypes.c_int, [ctypes.POINTER(MrgsTsdfConfig), c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_vertex_fuse": (ctypes.c_int, [ctypes.POINTER(MrgsVertexFuseConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_mesh_ws_bytes": (c_size_t, [ctypes.POINTER(MrgsMeshConfig)]),
    "mrgs_mesh_count": (ctypes.c_int, [ctypes.POINTER(MrgsMeshConfig), c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_mesh_emit": (ctypes.c_int, [ctypes.POINTER(MrgsMeshConfig), c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int64), c_void_p, c_void_p,
                                      c_void_p]),
    "mrgs_mesh_clusters": (ctypes.c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_mesh_select": (ctypes.c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "mrgs_mesh_reindex": (ctypes.c_int, [c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "mrgs_edges_ws_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_edge_mask": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "mrgs_knn_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_knn_mean_dist2": (ctypes.c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mrgs_mark_visible": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_envmap_lookup_forward": (ctypes.c_int, [ctypes.POINTER(MrgsEnvMips), c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_envmap_lookup_backward": (ctypes.c_int, [ctypes.POINTER(MrgsEnvMips), c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p]),
    "mrgs_shade_specular_forward": (ctypes.c_int, [ctypes.POINTER(MrgsEnvMips), ctypes.POINTER(MrgsShadeFrame), c_void_p, c_void_p,
                                                   c_void_p, c_void_p]),
    "mrgs_shade_specular_forward_composite": (ctypes.c_int, [ctypes.POINTER(MrgsEnvMips), ctypes.POINTER(MrgsShadeFrame), c_void_p, c_void_p, c_int32,
                                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "mrgs_shade_specular_backward": (ctypes.c_int, [ctypes.POINTER(MrgsEnvMips), ctypes.POINTER(MrgsShadeFrame), c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_surfel_shade_composite_backward": (ctypes.c_int, [ctypes.POINTER(MrgsEnvMips), ctypes.POINTER(MrgsShadeFrame), c_int32] + [c_void_p] * 13),
    "mrgs_bounce_shade_forward": (ctypes.c_int, [ctypes.POINTER(MrgsBounceConfig), ctypes.POINTER(MrgsEnvMips)] + [c_void_p] * 12),
    "mrgs_bounce_shade_backward": (ctypes.c_int, [ctypes.POINTER(MrgsBounceConfig), ctypes.POINTER(MrgsEnvMips)] + [c_void_p] * 14),
    "mrgs_debug_export": (ctypes.c_int, [ctypes.POINTER(MrgsRasterConfig), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                         c_void_p]),
    "mrgs_debug_sort_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_debug_radix_sort_pairs": (ctypes.c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "mrgs_debug_scan_ws_bytes": (c_size_t, [c_int64]),
    "mrgs_debug_scan_tiles": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mrgs_set_profiling": (ctypes.c_int, [c_int32]),
    "mrgs_get_kernel_times": (ctypes.c_int, [ctypes.POINTER(MrgsKernelTimes)]),
    "mrgs_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "mrgs_last_hip_error": (ctypes.c_char_p, []),
    "mrgs_version": (ctypes.c_char_p, []),
    "mrgs_abi_version": (c_int32, []),
    "mrgs_model_reset": (ctypes.c_int, [ctypes.POINTER(MrgsResetConfig), ctypes.POINTER(MrgsResetItem), c_int32, c_void_p]),
    "mrgs_lpips_weights_bytes": (c_size_t, []),
    "mrgs_lpips_pack_weights": (ctypes.c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_void_p, c_void_p]),
    "mrgs_lpips_ws_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "mrgs_lpips_ws_offsets": (ctypes.c_int, [c_int32, c_int32, ctypes.POINTER(c_size_t)]),
    "mrgs_lpips_forward": (ctypes.c_int, [ctypes.POINTER(MrgsLpipsConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_lpips_backward": (ctypes.c_int, [ctypes.POINTER(MrgsLpipsConfig), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_lpips_debug_conv": (ctypes.c_int, [ctypes.POINTER(MrgsLpipsConvConfig)] + [c_void_p] * 7 + [c_size_t, c_void_p]),
    "mrgs_lpips_debug_pool": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_lpips_debug_head": (ctypes.c_int, [c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                             c_void_p]),
    "mrgs_volume_features_ws_bytes": (c_size_t, []),
    "mrgs_volume_features_forward": (ctypes.c_int, [ctypes.POINTER(MrgsVolumeParams), ctypes.POINTER(MrgsEnvMips), ctypes.POINTER(MrgsEnvMips)] +
                                     [c_void_p] * 6),
    "mrgs_volume_features_backward": (ctypes.c_int, [ctypes.POINTER(MrgsVolumeParams), ctypes.POINTER(MrgsEnvMips), ctypes.POINTER(MrgsEnvMips)] +
                                      [c_void_p] * 5 + [ctypes.POINTER(MrgsVolumeGrads), c_void_p, c_void_p, c_size_t, c_void_p]),
    "mrgs_eval_metrics_ws_bytes": (c_size_t, [c_int32, c_int32]),
    "mrgs_eval_metrics": (ctypes.c_int, [ctypes.POINTER(MrgsEvalConfig), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_export_ws_bytes": (c_size_t, []),
    "mrgs_export_rgb8": (ctypes.c_int, [ctypes.POINTER(MrgsExportConfig), ctypes.POINTER(MrgsExportMap), c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_eval_jet_table": (ctypes.c_int, [c_void_p]),
    "mrgs_sheet_ws_bytes": (c_size_t, []),
    "mrgs_sheet_rgb8": (ctypes.c_int, [ctypes.POINTER(MrgsSheetConfig), ctypes.POINTER(MrgsSheetCell), c_void_p, c_size_t, c_void_p, c_void_p]),
    "mrgs_ball_query_ws_bytes": (c_size_t, [c_int64, c_int64]),
    "mrgs_ball_query": (ctypes.c_int, [c_float, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mrgs_furthest_point_sample": (ctypes.c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mrgs_depth_points": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "mrgs_ball_max_pool": (ctypes.c_int, [c_float, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_size_t,
                                          c_void_p]),
    "mrgs_image_resize_ws_bytes": (c_size_t, [c_int32] * 5),
    "mrgs_image_resize_u8": (ctypes.c_int, [ctypes.POINTER(MrgsResizeConfig)] + [c_void_p] * 6 + [c_size_t, c_void_p, c_void_p]),
    "mrgs_image_composite_u8": (ctypes.c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mrgs_view_decode": (ctypes.c_int, [ctypes.POINTER(MrgsViewDecode), c_void_p]),
}
MRGS_ABI_VERSION = 10   # the revision of include/mrgs.h these ctypes declarations were written against

_lib = None


def build(force=False):
    """Compile libmrgs.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", _CSRC, "-s", "-j8"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built (run `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C materialrefgs_amd/csrc`). There is no CPU fallback for the rasterizer.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)   # AttributeError here = the library does not export what mrgs.h declares
            fn.restype = res
            fn.argtypes = args
        if L.mrgs_abi_version() != MRGS_ABI_VERSION:
            raise ImportError(f"{LIB_PATH} implements ABI revision {L.mrgs_abi_version()} of include/mrgs.h, this binding was written "
                              f"against revision {MRGS_ABI_VERSION}: rebuild the library (make -C materialrefgs_amd/csrc)")
        _lib = L
    return _lib


# the status codes of include/mrgs.h
(MRGS_OK, MRGS_E_BAD_ARG, MRGS_E_TOO_MANY_FEATURES, MRGS_E_NEED_COLORS, MRGS_E_HIP, MRGS_E_WORKSPACE, MRGS_E_UNSUPPORTED,
 MRGS_E_INTERNAL) = range(8)


# ---- launch plumbing (host time per call matters: a full render is ~30 native calls a view) -----------------------------------------
class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()
_current_device = torch._C._cuda_getDevice                 # int
_raw_stream = torch._C._cuda_getCurrentRawStream           # (device index) -> the hipStream_t of torch's current stream, as an int


def guard(dev):
    """`with guard(dev):` -- torch.cuda.device(dev) only when `dev` is not already the current device (the usual case: one process, one
    GPU), otherwise nothing: the device context costs ~4 us a time, a view enters it ~25 times."""
    idx = dev.index
    return _NO_GUARD if (idx is None or idx == _current_device()) else torch.cuda.device(dev)


def stream_ptr(dev):
    """torch's current stream on `dev` as the integer handle the C ABI's `void* stream` arguments take (ctypes converts)."""
    idx = dev.index
    return _raw_stream(_current_device() if idx is None else idx)


def f32c(t):
    """detached float32 contiguous view of `t` (itself when it already is one: the common case costs two attribute reads)."""
    if t.dtype is torch.float32 and t.is_contiguous():
        return t.detach() if t.requires_grad else t
    return t.detach().to(torch.float32).contiguous()


def ptr(t):
    """Address of a tensor's data as an int, None (NULL) for None: ctypes converts either for the `void*` parameters and struct fields.
    (An empty tensor's address 0 is NULL as well.)"""
    return None if t is None else t.data_ptr()


def check(rc):
    if rc != 0:
        L = lib()
        msg = L.mrgs_strerror(rc).decode()
        if rc == MRGS_E_HIP:
            msg += ": " + L.mrgs_last_hip_error().decode()
        raise RuntimeError(f"libmrgs: {msg}")
