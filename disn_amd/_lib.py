"""ctypes binding of libdisn_amd.so (include/disn_amd.h and, for the mesh simplification and the vertex colours,
include/disn_amd_simplify.h and include/disn_amd_colour.h; for the surface samples, include/disn_amd_sample.h; for
the Taubin smoothing, include/disn_amd_smooth.h; for dual contouring, include/dc/disn_amd_dc.h and
include/dc/disn_amd_dc_sheets.h; for the mesh checks, include/check/disn_amd_check.h; for the mesh repair,
include/repair/disn_amd_repair.h; for the mesh closing, include/close/disn_amd_close.h).

The HIP library is the product: there is NO CPU fallback.  ``lib()`` raises
``DisnLibraryError`` when the shared object is missing or does not export the
ABI this package was written against; every wrapper raises ``DisnError`` on a
non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
# DISN_AMD_LIB: tools/ only -- points the binding at a tuning build (csrc/build.py --tuning), never set by the product
LIB_PATH = os.environ.get("DISN_AMD_LIB") or os.path.join(HERE, "csrc", "libdisn_amd.so")
ABI_VERSION = 10

c_float_p = C.c_void_p  # device pointers travel as integers (tensor.data_ptr())


class DisnLibraryError(RuntimeError):
    pass


class DisnError(RuntimeError):
    def __init__(self, fn: str, status: int):
        kind = {-1: "invalid argument", -2: "unsupported shape", -3: "workspace too small",
                -4: "did not converge"}.get(
            status, "hipError_t %d" % status if status > 0 else "error")
        super().__init__("%s failed: %s (status %d)" % (fn, kind, status))
        self.status = status


class VggWeights(C.Structure):  # disn_vgg_weights_t
    _fields_ = [("conv_w", C.c_void_p * 13), ("conv_b", C.c_void_p * 13),
                ("fc_w", C.c_void_p * 3), ("fc_b", C.c_void_p * 3), ("num_classes", C.c_int),
                ("conv_w_x3", C.c_void_p * 13),   # optional three-term bf16 images (disn_pack_kn_x3)
                ("conv_w_h2", C.c_void_p * 13),   # optional two-term f16 images (disn_pack_conv_h2)
                ("fc_w_t", C.c_void_p * 3),       # optional transposed fc matrices [N][K]
                ("strict_forms", C.c_int)]           # 1: single-image convolution kernels for every call size ("strict")


MLP_FIELDS = ("g_w1", "g_b1", "g_w2", "g_b2", "g_w3", "g_b3", "g_w4_point", "g_w4_global", "g_b4",
              "g_w5", "g_b5", "g_w6", "g_b6", "l_w1", "l_b1", "l_w2", "l_b2", "l_w3", "l_b3",
              "l_w4", "l_b4", "l_w5", "l_b5", "l_w6", "l_b6")


MLP_X3_FIELDS = ("g_x2", "g_x3", "g_x4_point", "g_x5", "l_x2", "l_x3", "l_x4", "l_x5")   # optional
MLP_FOLD_FIELDS = ("l_w4_point", "l_w4_feat", "l_x4_point", "l_x4_feat")   # optional: *_folded entry points
MLP_FUSED_FIELDS = ("g_fused", "l_fused")   # optional: *_fused entry points (disn_mlp_fused_pack images)
MLP_T_FIELDS = ("g_w4_global_t",)           # optional: g_w4_global transposed [512][1024]
MLP_D_FIELDS = ("g_d2", "g_d3", "g_d4_point", "g_d5", "l_d2", "l_d3", "l_d4", "l_d5")   # optional: dense_h2 images
MLP_FEAT_FIELDS = ("l_feat",)               # optional: disn_mlp_fused_feat_pack image (fused small-set local stream)


class MlpWeights(C.Structure):  # disn_mlp_weights_t
    _fields_ = [(n, C.c_void_p) for n in MLP_FIELDS + MLP_X3_FIELDS + MLP_FOLD_FIELDS + MLP_FUSED_FIELDS + MLP_T_FIELDS + MLP_D_FIELDS + MLP_FEAT_FIELDS]


CAM_FIELDS = tuple("%s_%s%d" % (t, k, i) for t in "srt" for i in (1, 2, 3) for k in "wb")


class CamWeights(C.Structure):  # disn_cam_weights_t: s_w1, s_b1, s_w2, ... t_b3
    _fields_ = [(n, C.c_void_p) for n in CAM_FIELDS]


class EqWeights(C.Structure):  # disn_eq_weights_t (HOST pointers, modified in place)
    _fields_ = [("conv_w", C.c_void_p * 13), ("conv_b", C.c_void_p * 13), ("fc6_w", C.c_void_p),
                ("mlp_w", (C.c_void_p * 6) * 2), ("mlp_b", (C.c_void_p * 6) * 2), ("num_classes", C.c_int)]


NUM_VARS = 56


class ParamLayout(C.Structure):  # disn_param_layout_t
    _fields_ = [("offset", C.c_int64 * NUM_VARS), ("count", C.c_int64 * NUM_VARS), ("total", C.c_int64)]


CAM_NUM_VARS = 50


class CamParamLayout(C.Structure):  # disn_cam_param_layout_t
    _fields_ = [("offset", C.c_int64 * CAM_NUM_VARS), ("count", C.c_int64 * CAM_NUM_VARS), ("total", C.c_int64)]


# name -> (restype, argtypes); every symbol declared in include/disn_amd.h
I, Z, P, F, L = C.c_int, C.c_size_t, C.c_void_p, C.c_float, C.c_int64
SIGNATURES = {
    "disn_abi_version": (I, []),
    "disn_pack_kn": (I, [P, I, I, I, P, P]),
    "disn_pack_kn_x3_bytes": (Z, [I, I]),
    "disn_pack_kn_x3": (I, [P, I, I, P, P]),
    "disn_conv3x3_x3_workspace_bytes": (Z, [I, I, I, I, I]),
    "disn_conv3x3_x3": (I, [P, I, I, I, I, P, P, I, I, P, P, Z, P]),
    "disn_pack_conv_h2_bytes": (Z, [I, I]),
    "disn_pack_conv_h2": (I, [P, I, I, P, P]),
    "disn_conv_h2_gain_span": (I, [P, I, I, P, P]),
    "disn_conv1_1_workspace_bytes": (Z, []),
    "disn_conv1_1": (I, [P, I, I, I, P, P, I, P, P, P, Z, P]),
    "disn_conv3x3_h2_workspace_bytes": (Z, [I]),
    "disn_conv3x3_h2": (I, [P, I, I, I, I, P, P, I, I, P, P, P, I, P, Z, P]),
    "disn_conv3x3_h2_plan": (I, [I, I, I, I, I, I, P, P]),
    "disn_resize_bilinear": (I, [P, I, I, I, I, P, I, I, I, I, P]),
    "disn_vgg16_workspace_bytes": (Z, [I]),
    "disn_vgg16_forward": (I, [C.POINTER(VggWeights), P, I, P, C.POINTER(C.c_void_p * 5), P, P, Z, P]),
    "disn_vgg16_conv_stack": (I, [C.POINTER(VggWeights), P, I, P, C.POINTER(C.c_void_p * 5), P, P, Z, P]),
    "disn_conv3x3_workspace_bytes": (Z, [I, I, I, I, I]),
    "disn_conv3x3": (I, [P, I, I, I, I, P, P, I, I, P, P, Z, P]),
    "disn_conv3x3_planned_workspace_bytes": (Z, [I, I, I, I, I, I, I, I]),
    "disn_conv3x3_planned": (I, [P, I, I, I, I, P, P, I, I, P, P, Z, I, I, I, P]),
    "disn_maxpool2x2": (I, [P, I, I, I, I, P, P]),
    "disn_fc_workspace_bytes": (Z, [I, I, I]),
    "disn_fc": (I, [P, I, I, P, P, I, I, P, P, Z, P]),
    "disn_pack_dense_h2_bytes": (Z, [I, I]),
    "disn_pack_dense_h2": (I, [P, I, I, P, P]),
    "disn_dense_h2_workspace_bytes": (Z, [I]),
    "disn_dense_h2": (I, [P, I, I, P, I, I, P, I, I, P, I, I, P, P, I, I, P, P, P, Z, P]),
    "disn_get_loss": (I, [P, P, L, F, F, P, P]),
    "disn_fc_t": (I, [P, I, I, P, P, I, I, P, P]),
    "disn_dense_workspace_bytes": (Z, [I, I, I]),
    "disn_dense": (I, [P, I, I, P, I, I, I, P, P, I, I, P, P, Z, P]),
    "disn_build_featmap": (I, [C.POINTER(C.c_void_p * 5), I, P, P]),
    "disn_project": (I, [P, P, I, I, P, P]),
    "disn_gather": (I, [P, P, I, I, P, P]),
    "disn_gather_taps": (I, [C.POINTER(C.c_void_p * 5), P, P, I, I, P, P]),
    "disn_gather_taps_split": (I, [C.POINTER(C.c_void_p * 5), P, P, I, I, P, P, P]),
    "disn_gather_fold": (I, [P, P, P, I, P, P, P, P]),
    "disn_mlp_fused_image_bytes": (Z, []),
    "disn_mlp_fused_pack": (I, [P, P, P, P, P, P]),
    "disn_mlp_fused_feat_image_bytes": (Z, []),
    "disn_mlp_fused_feat_pack": (I, [P, P, P, P, P, P]),
    "disn_query_taps_fused_workspace_bytes": (Z, [I, I]),
    "disn_query_taps_fused": (I, [C.POINTER(MlpWeights), C.POINTER(C.c_void_p * 5), P, P, P, P, I, I, P, P, Z, P]),
    "disn_amax": (I, [P, L, P, P]),
    "disn_query_fused_workspace_bytes": (Z, [I, L]),
    "disn_query_fused": (I, [C.POINTER(MlpWeights), P, P, P, P, P, P, I, L, P, P, Z, P]),
    "disn_query_grid_fused_workspace_bytes": (Z, [L]),
    "disn_query_grid_fused": (I, [C.POINTER(MlpWeights), P, P, P, P, C.POINTER(C.c_double * 6), I, L, L, F, P,
                                  P, Z, P]),
    "disn_query_grid_listed_workspace_bytes": (Z, [L]),
    "disn_query_grid_listed": (I, [C.POINTER(MlpWeights), P, P, P, P, C.POINTER(C.c_double * 6), I, P, I, L, L, F, P,
                                   P, Z, P]),
    "disn_grid_band_select_workspace_bytes": (Z, [I, I]),
    "disn_grid_band_select": (I, [P, I, I, F, F, I, P, P, L, P, P, Z, P]),
    "disn_grid_band_fill": (I, [P, I, I, P, P]),
    "disn_sdf_mlp_workspace_bytes": (Z, [I, I]),
    "disn_sdf_mlp": (I, [C.POINTER(MlpWeights), P, P, P, I, I, P, P, P, P, Z, P]),
    "disn_query_workspace_bytes": (Z, [I, I]),
    "disn_query": (I, [C.POINTER(MlpWeights), P, P, P, P, P, I, I, P, P, Z, P]),
    "disn_stream_create": (I, [C.POINTER(C.c_void_p)]),
    "disn_stream_destroy": (I, [P]),
    "disn_ctx_create": (I, [C.POINTER(C.c_void_p)]),
    "disn_ctx_destroy": (I, [P]),
    "disn_ctx_pipeline": (I, [P, P, P]),
    "disn_encode_workspace_bytes": (Z, [I]),
    "disn_encode": (I, [P, C.POINTER(VggWeights), P, I, P, C.POINTER(C.c_void_p * 5), P, P, P, Z, P]),
    "disn_encode_query_workspace_bytes": (Z, [I, I]),
    "disn_encode_query": (I, [P, C.POINTER(VggWeights), C.POINTER(MlpWeights), P, P, P, P, I, I, P,
                              C.POINTER(C.c_void_p * 5), P, P, P, P, Z, P]),
    "disn_query_grid_ctx_workspace_bytes": (Z, [L]),
    "disn_query_grid_ctx": (I, [P, C.POINTER(MlpWeights), P, P, P, C.POINTER(C.c_double * 6), I, L, L, F, P,
                                P, Z, P]),
    "disn_crc32c": (C.c_uint32, [P, Z, C.c_uint32]),
    "disn_equalise_weights": (I, [C.POINTER(EqWeights), P, P]),
    "disn_scale_channels": (I, [P, L, I, P, I, P, P]),
    "disn_dense_bf16_workspace_bytes": (Z, [I, I, I]),
    "disn_dense_bf16": (I, [P, I, I, P, I, I, I, P, P, I, I, I, P, P, Z, P]),
    "disn_conv3x3_bf16_workspace_bytes": (Z, [I, I, I, I, I]),
    "disn_conv3x3_bf16": (I, [P, I, I, I, I, P, P, I, I, I, P, P, Z, P]),
    "disn_cam_head": (I, [C.POINTER(CamWeights), P, C.POINTER(C.c_float * 9), I, P, P, P, P, P]),
    "disn_param_layout": (I, [C.POINTER(ParamLayout)]),
    "disn_cam_param_layout": (I, [C.POINTER(CamParamLayout)]),
    "disn_cam_train_workspace_bytes": (Z, [I, I]),
    "disn_cam_train_step": (I, [P, P, P, P, P, P, P, C.POINTER(C.c_float * 9), I, I, F, I, I, P, P, P, P, Z, P]),
    "disn_cam_loss_backward_workspace_bytes": (Z, [I, I]),
    "disn_cam_loss_backward": (I, [C.POINTER(CamWeights), P, C.POINTER(C.c_float * 9), P, P, P, I, I, I, P, P, P,
                                   P, P, P, P, Z, P]),
    "disn_train_workspace_bytes": (Z, [I, I]),
    "disn_train_step": (I, [P, P, P, P, P, P, P, P, I, I, F, F, F, I, P, P, P, P, Z, P]),
    "disn_adam_update": (I, [P, P, P, P, L, F, F, F, F, F, P]),
    "disn_dense_backward_workspace_bytes": (Z, [I, I, I]),
    "disn_dense_backward": (I, [P, I, I, P, P, P, I, I, F, I, P, P, P, P, Z, P]),
    "disn_conv3x3_backward_workspace_bytes": (Z, [I, I, I, I, I]),
    "disn_conv3x3_backward": (I, [P, I, I, I, I, P, P, P, I, F, I, P, P, P, P, Z, P]),
    "disn_maxpool2x2_backward": (I, [P, P, I, I, I, I, P, P]),
    "disn_resize_bilinear_backward_workspace_bytes": (Z, [I, I, I, I, I, I]),
    "disn_resize_bilinear_backward": (I, [P, I, I, I, I, I, I, I, I, P, I, P, Z, P]),
    "disn_gather_backward": (I, [P, P, I, I, P, P]),
    "disn_mc_workspace_bytes": (Z, [I]),
    "disn_mc_count": (I, [P, I, F, P, P, Z, P]),
    "disn_mc_emit": (I, [P, C.POINTER(C.c_double * 6), I, F, P, P, P, Z, P]),
    "disn_mc_batch_workspace_bytes": (Z, [I, I]),
    "disn_mc_count_batch": (I, [P, I, I, F, P, P, Z, P]),
    "disn_mc_emit_batch": (I, [P, P, I, I, F, P, P, P, Z, P]),
    "disn_write_obj": (I, [C.c_char_p, P, L, P, L]),
    "disn_write_obj_normals": (I, [C.c_char_p, P, L, P, P, L]),
    "disn_read_obj_verts": (L, [C.c_char_p, P, L]),
    "disn_read_obj_mesh": (I, [C.c_char_p, P, L, P, L, P]),
    "disn_mesh_bvh_bytes": (Z, [L]),
    "disn_mesh_bvh_build": (I, [P, L, P, L, P, Z]),
    "disn_mesh_udf_points": (I, [P, L, P, L, I, P, P]),
    "disn_mesh_udf_grid": (I, [P, L, P, P, P, I, I, I, I, P, P]),
    "disn_mesh_sign_workspace_bytes": (Z, [I, I, I]),
    "disn_mesh_sign": (I, [P, L, P, P, P, I, I, I, P, F, I, F, P, P, P, Z, P]),
    "disn_mesh_bvh_build_order": (I, [P, L, P, L, P, Z, P]),
    "disn_render_views": (I, [P, L, P, P, P, I, I, I, I, F, I, P, P, P, P]),
    "disn_trace_state_bytes": (Z, [L]),
    "disn_trace_setup": (I, [P, I, I, I, C.POINTER(C.c_double * 6), F, P, Z, P, P]),
    "disn_trace_advance": (I, [P, I, I, I, P, L, I, F, F, F, F, F, F, I, I, P, Z, P, P]),
    "disn_trace_collect": (I, [P, I, I, I, P, Z, P, P]),
    "disn_trace_shade": (I, [P, I, I, I, P, Z, P, P, L, F, F, F, P, P, P, P, P, P]),
    "disn_mesh_components": (I, [P, L, L, I, P, C.POINTER(C.c_int64)]),
    "disn_voxel_grid_words": (Z, [I]),
    "disn_voxel_surface_workspace_bytes": (Z, [L]),
    "disn_voxel_surface": (I, [P, L, P, L, I, I, I, P, P, P, Z, P]),
    "disn_voxel_fill_workspace_bytes": (Z, [I]),
    "disn_voxel_fill": (I, [P, I, P, P, Z, P]),
    "disn_voxel_index_grid": (I, [P, I, P, I, P, P]),
    "disn_voxel_iou": (I, [P, P, I, L, P, P, P]),
    "disn_assemble_batch": (I, [P, P, L, P, P, P, L, P, P, P, I, I, I, I, P, P, P, P, P, P, P]),
    "disn_metrics_workspace_bytes": (Z, [I, I, I]),
    "disn_nn_distance": (I, [P, P, I, I, I, P, P, P, P, P, Z, P]),
    "disn_approx_match": (I, [P, P, I, I, I, P, P, Z, P]),
    "disn_match_cost": (I, [P, P, P, I, I, I, P, P, Z, P]),
    "disn_emd": (I, [P, P, I, I, I, P, P, Z, P]),
    "disn_grid_points": (I, [C.POINTER(C.c_double * 6), I, L, L, P, P]),
    "disn_query_grid_workspace_bytes": (Z, [L]),
    "disn_query_grid": (I, [C.POINTER(MlpWeights), P, P, P, C.POINTER(C.c_double * 6), I, L, L, F, P,
                            P, Z, P]),
    "disn_fold_local_workspace_bytes": (Z, []),
    "disn_fold_local": (I, [C.POINTER(MlpWeights), P, P, P, Z, P]),
    "disn_query_folded": (I, [C.POINTER(MlpWeights), P, P, P, P, P, I, I, P, P, Z, P]),
    "disn_query_grid_folded": (I, [C.POINTER(MlpWeights), P, P, P, C.POINTER(C.c_double * 6), I, L, L, F, P,
                                   P, Z, P]),
    "disn_gather_taps_pool": (I, [C.POINTER(C.c_void_p * 5), I, P, P, I, P, I, P, P]),
    "disn_pool_embedding": (I, [P, I, P, I, P, P]),
    "disn_query_views_workspace_bytes": (Z, [I]),
    "disn_query_views": (I, [C.POINTER(MlpWeights), C.POINTER(C.c_void_p * 5), I, P, P, P, I, P, I, P, P, Z, P]),
    "disn_query_grid_views_workspace_bytes": (Z, [I]),
    "disn_query_grid_views": (I, [C.POINTER(MlpWeights), C.POINTER(C.c_void_p * 5), I, P, P, P, I,
                                  C.POINTER(C.c_double * 6), I, L, L, F, P, P, Z, P]),
    "disn_query_grad_workspace_bytes": (Z, [I, L]),
    "disn_query_grad": (I, [C.POINTER(MlpWeights), P, P, P, P, I, L, P, P, P, Z, P]),
    "disn_mesh_clean_workspace_bytes": (Z, [I, L, L]),
    "disn_mesh_components_device": (I, [P, P, P, P, I, I, P, P, P, P, Z, P]),
    "disn_mesh_clean_count_batch": (I, [P, P, P, P, I, I, C.c_double, C.c_double, P, P, Z, P]),
    "disn_mesh_clean_emit_batch": (I, [P, P, P, P, P, I, P, P, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/disn_amd_simplify.h (the second header of the same
# library: include/disn_amd.h, SIGNATURES and the ABI version stay as they are)
SIGNATURES_SIMPLIFY = {
    "disn_mesh_simplify_workspace_bytes": (Z, [I, L, L]),
    "disn_mesh_simplify_count_batch": (I, [P, P, P, P, P, P, I, I, P, P, Z, P]),
    "disn_mesh_simplify_emit_batch": (I, [P, P, P, P, I, P, P, P, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/disn_amd_colour.h (the third header, added the same way)
SIGNATURES_COLOUR = {
    "disn_mesh_colour_workspace_bytes": (Z, [I, I, L, L, I]),
    "disn_mesh_zbuffer_batch": (I, [P, P, P, P, I, P, I, I, P, P, P, Z, P]),
    "disn_mesh_colour_batch": (I, [P, P, P, P, I, P, P, P, I, I, F, I, I, I, P, P, P, P, Z, P]),
    "disn_write_obj_colours": (I, [C.c_char_p, P, L, P, P, P, L]),
}

# name -> (restype, argtypes); every symbol declared in include/disn_amd_sample.h (the fourth header, added the same way)
SIGNATURES_SAMPLE = {
    "disn_mesh_sample_workspace_bytes": (Z, [I, L, L, I]),
    "disn_mesh_sample_batch": (I, [P, P, P, P, I, P, I, P, P, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/disn_amd_smooth.h (the fifth header, added the same way)
D = C.c_double
SIGNATURES_SMOOTH = {
    "disn_mesh_smooth_workspace_bytes": (Z, [I, L, L]),
    "disn_mesh_smooth_batch": (I, [P, P, P, P, I, I, D, D, I, P, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/dc/disn_amd_dc.h (the sixth header, one directory below
# the other five: dual contouring beside disn_mc_*_batch)
SIGNATURES_DC = {
    "disn_dc_workspace_bytes": (Z, [I, I]),
    "disn_dc_count_batch": (I, [P, I, I, F, P, P, Z, P]),
    "disn_dc_points_batch": (I, [P, P, I, I, F, P, P, Z, P]),
    "disn_dc_grid_normals_batch": (I, [P, P, I, I, F, P, P, Z, P]),
    "disn_dc_emit_batch": (I, [P, P, I, I, F, P, P, D, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/dc/disn_amd_dc_sheets.h (the seventh header, beside the
# sixth: per-sheet dual contouring, the argument lists of disn_dc_*)
SIGNATURES_DCS = {name.replace("disn_dc_", "disn_dcs_"): sig for name, sig in SIGNATURES_DC.items()}

# name -> (restype, argtypes); every symbol declared in include/check/disn_amd_check.h (the eighth header, in a
# directory of its own as the sixth and seventh: the mesh checks)
SIGNATURES_CHECK = {
    "disn_mesh_check_workspace_bytes": (Z, [I, L, L, L]),
    "disn_mesh_check_batch": (I, [P, P, P, P, I, P, P, P, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/repair/disn_amd_repair.h (the ninth header, in a
# directory of its own: the mesh repair)
SIGNATURES_REPAIR = {
    "disn_mesh_repair_workspace_bytes": (Z, [I, L, L]),
    "disn_mesh_repair_count_batch": (I, [P, P, P, P, I, I, P, P, Z, P]),
    "disn_mesh_repair_emit_batch": (I, [P, P, P, P, I, I, P, P, P, P, P, P, Z, P]),
}

# name -> (restype, argtypes); every symbol declared in include/close/disn_amd_close.h (the tenth header: the mesh
# closing)
SIGNATURES_CLOSE = {
    "disn_mesh_close_workspace_bytes": (Z, [I, L, L]),
    "disn_mesh_close_count_batch": (I, [P, P, P, P, I, I, L, P, P, Z, P]),
    "disn_mesh_close_emit_batch": (I, [P, P, P, P, I, I, L, P, P, P, P, P, P, Z, P]),
}

_LIB: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and type the shared library.  Fails loudly."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise DisnLibraryError(
            "HIP extension %s is missing: build it with `python -m disn_amd.csrc.build` "
            "(or __graft_entry__.build()).  There is no CPU fallback." % LIB_PATH)
    try:
        h = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the box
        raise DisnLibraryError("cannot load %s: %s" % (LIB_PATH, e)) from e
    for name, (res, args) in [kv for t in (SIGNATURES, SIGNATURES_SIMPLIFY, SIGNATURES_COLOUR, SIGNATURES_SAMPLE,
                                                     SIGNATURES_SMOOTH, SIGNATURES_DC, SIGNATURES_DCS, SIGNATURES_CHECK,
                                                     SIGNATURES_REPAIR, SIGNATURES_CLOSE) for kv in t.items()]:
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise DisnLibraryError("%s does not export %s" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    v = h.disn_abi_version()
    if v != ABI_VERSION:
        raise DisnLibraryError("ABI mismatch: library %d, binding %d" % (v, ABI_VERSION))
    _LIB = h
    return h


def check(fn: str, status: int) -> None:
    if status != 0:
        raise DisnError(fn, status)
