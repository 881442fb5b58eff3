"""ctypes binding of the C-ABI declared in include/unidepth_hip.h (libunidepth_hip.so, built in-tree by
unidepth_amd/csrc/build.sh).  There is NO fallback: if the library is missing the import fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UNIDEPTH_HIP_LIB", os.path.join(_HERE, "libunidepth_hip.so"))   # env override: A/B two builds in one process tree

UD_EPI_F16, UD_EPI_F32, UD_EPI_QKV, UD_EPI_D2S, UD_EPI_HEAD = 0, 1, 2, 3, 4
UD_ACT_NONE, UD_ACT_GELU, UD_ACT_LRELU = 0, 1, 2
UD_A_DENSE, UD_A_CONV3_ZERO, UD_A_CONV3_REFLECT, UD_A_CONV3_REFLECT_UP = 0, 1, 2, 3
# UdGemm.tile_hint and the codes / flags of ud_gemm_pick (include/unidepth_hip.h)
UD_HINT_AUTO, UD_HINT_TILE128, UD_HINT_LIST256, UD_HINT_LIST192 = 0, 1, 2, 3
UD_HINT_PLAIN128, UD_HINT_RING, UD_HINT_RING_SPLITK, UD_HINT_BALANCED, UD_HINT_LIST192_W2, UD_HINT_LIST192_SPLITK = 5, 6, 7, 8, 9, 10
UD_HINT_PINGPONG, UD_HINT_DUO_FIRST, UD_HINT_DUO_EQUAL, UD_HINT_DUO_SECOND = 11, 12, 13, 14
UD_PICK_TILE128, UD_PICK_TILE128_BN64, UD_PICK_TILE128_BN32, UD_PICK_LIST192, UD_PICK_LIST256, UD_PICK_CONV_TILE = 0, 1, 2, 3, 4, 5
UD_PICK_RING, UD_PICK_RING_SPLITK, UD_PICK_BALANCED, UD_PICK_LIST192_SPLITK, UD_PICK_PINGPONG, UD_PICK_DUO = 6, 7, 8, 10, 11, 12
UD_PICK_SCHEDULE, UD_PICK_LN_CONSUMER, UD_PICK_GROUPED = 15, 16, 32
UD_PICK_LARGE_TILE = (UD_PICK_LIST192, UD_PICK_LIST256, UD_PICK_BALANCED)     # the schedules that take a folded-LayerNorm consumer

vp, fp, i32, i64, f32 = C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_float


class UdGemm(C.Structure):
    _fields_ = [
        ("A", vp), ("W", vp), ("bias", fp), ("out", vp), ("out2", vp), ("add", fp), ("zeros", vp), ("w2", fp),
        ("M", i32), ("N", i32), ("K", i32),
        ("lda", i32), ("ldw", i32), ("ldc", i32), ("ldc2", i32), ("ldadd", i32),
        ("amode", i32), ("epi", i32), ("act", i32), ("act2", i32), ("accumulate", i32),
        ("rows_in", i32), ("rows_out", i32), ("row_off", i32), ("add_row_off", i32),
        ("Himg", i32), ("Wimg", i32), ("Cin", i32), ("cstride", i32), ("coff", i32), ("rows_img", i32),
        ("img_stride", i64),
        ("vsplit", i32), ("tok_per_img", i32), ("kv_ld", i32), ("heads_v", i32),
        ("d2s_k", i32), ("d2s_Co", i32), ("d2s_Hin", i32), ("d2s_Win", i32), ("d2s_rows_in_img", i32),
        ("d2s_out_img_pix", i64),
        ("b2", f32), ("post_add", f32),
        ("groups", i32),
        ("gA", i64), ("gW", i64), ("gBias", i64), ("gOut", i64), ("gOut2", i64), ("gW2", i64),
        ("b2_g1", f32), ("post_add_g1", f32), ("tile_hint", i32),
        ("splitk_ws", vp), ("splitk_cnt", vp), ("Hsrc", i32), ("Wsrc", i32), ("a_wrap", i32), ("w_wrap", i32), ("max_out", fp), ("max_init", i32), ("grp_rows", i32),
        ("row_stats_out", fp), ("row_stats_final", fp), ("row_stats_ticket", vp), ("row_stats_in", fp), ("wsum", fp), ("ln_slabs", i32), ("ln_D", i32), ("ln_eps", f32),
        ("up_src", fp), ("up_H", i32), ("up_W", i32), ("up_ld", i32), ("up_img_rows", i32),
        ("splitk_ws_bytes", i64),
    ]


class UdLayerNorm(C.Structure):
    _fields_ = [("x", fp), ("y", vp), ("rows", i32), ("D", i32), ("ldx", i32), ("ldy", i32), ("eps", f32),
                ("rows_per_img", i32), ("in_rows_per_img", i32), ("in_row_off", i32), ("out_rows_per_img", i32),
                ("out_row_off", i32), ("out_f32", i32), ("gamma", fp), ("beta", fp), ("add", fp), ("cls_y", fp), ("ldcls", i32)]


class UdLinearF32(C.Structure):
    _fields_ = [("x", fp), ("W", fp), ("bias", fp), ("add", fp), ("out", fp), ("M", i32), ("N", i32), ("K", i32), ("ldx", i32),
                ("ldw", i32), ("ldc", i32), ("ldadd", i32), ("add_mod", i32), ("act", i32), ("accumulate", i32)]


class UdCamPhase(C.Structure):
    _fields_ = [("x", fp), ("W", fp), ("bias", fp), ("add", fp), ("out", fp), ("M", i32), ("N", i32), ("K", i32), ("ldx", i32), ("ldc", i32),
                ("ldadd", i32), ("add_mod", i32), ("add_cols", i32), ("kind", i32), ("ln", i32), ("act", i32), ("accumulate", i32), ("sync", i32)]


UD_CAM_MAX_PHASES = 24


class UdCameraHead(C.Structure):
    _fields_ = [("ph", UdCamPhase * UD_CAM_MAX_PHASES), ("n_phases", i32), ("T", i32), ("H", i32), ("C", i32), ("scale", f32), ("eps", f32),
                ("sync_ws", vp), ("workgroups", i32), ("fail_host", vp), ("spin_limit", C.c_uint)]


class UdDwConv7(C.Structure):
    _fields_ = [("x", fp), ("w", fp), ("bias", fp), ("y", fp), ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("ldx", i32), ("ldy", i32),
                ("y16", vp), ("stats_out", fp), ("ldy16", i32), ("stats_final", fp), ("stats_ticket", vp), ("ln_eps", f32)]


class UdV1Op(C.Structure):
    _fields_ = [("kind", i32), ("a", vp), ("b", vp), ("c", vp), ("out", vp), ("out2", vp), ("i", i32 * 12), ("f", f32 * 4)]


class UdKnn(C.Structure):
    _fields_ = [("p1", vp), ("p2", vp), ("lengths1", vp), ("lengths2", vp), ("dists", vp), ("idx", vp), ("work", vp),
                ("N", i32), ("P1", i32), ("P2", i32), ("D", i32), ("K", i32), ("norm", i32)]


class UdExtractPatches(C.Structure):
    _fields_ = [("in_", vp), ("out", vp), ("centers", vp), ("B", i32), ("C", i32), ("H", i32), ("W", i32), ("N", i32),
                ("h", i32), ("w", i32), ("pad_h", i32), ("pad_w", i32)]


class UdEvalDepth(C.Structure):
    _fields_ = [("gt", vp), ("pred", vp), ("mask", vp), ("thresholds", vp), ("out", vp), ("work", vp),
                ("B", i32), ("H", i32), ("W", i32), ("h", i32), ("w", i32), ("max_depth", f32), ("has_max_depth", i32),
                ("work_bytes", i64)]


UD_EVAL3D_MAX_B, UD_EVAL3D_MAX_T = 32767, 1024


class UdEval3d(C.Structure):
    _fields_ = [("gt", vp), ("pred", vp), ("mask", vp), ("thresholds", vp), ("out", vp), ("counts", vp), ("size", vp),
                ("work", vp), ("work_bytes", i64), ("B", i32), ("H", i32), ("W", i32), ("T", i32)]


UD_RECON_MAX_B = 256


class UdReconstruct(C.Structure):
    _fields_ = [("depth", vp), ("params", vp), ("points", vp), ("work", vp), ("work_bytes", i64), ("B", i32), ("H", i32), ("W", i32),
                ("model", C.c_ubyte * UD_RECON_MAX_B)]


class UdCameraProject(C.Structure):
    _fields_ = [("xyz", vp), ("params", vp), ("T", vp), ("uv", vp), ("inside", vp), ("depth", vp),
                ("batch_stride", i64), ("point_stride", i64), ("comp_stride", i64), ("n_points", i64),
                ("B", i32), ("H", i32), ("W", i32), ("nT", i32), ("uv_rows", i32), ("model", C.c_ubyte * UD_RECON_MAX_B)]


class UdCameraUnproject(C.Structure):
    _fields_ = [("uv", vp), ("params", vp), ("depth", vp), ("rays", vp), ("valid", vp), ("work", vp), ("work_bytes", i64),
                ("batch_stride", i64), ("point_stride", i64), ("comp_stride", i64), ("n_points", i64),
                ("B", i32), ("H", i32), ("W", i32), ("normalize", i32), ("rays_rows", i32), ("model", C.c_ubyte * UD_RECON_MAX_B)]


UD_REMAP_NEAREST, UD_REMAP_BILINEAR = 0, 1
UD_REMAP_ZEROS, UD_REMAP_BORDER = 0, 1


class UdRemap(C.Structure):
    _fields_ = [("src", vp), ("src_mask", vp), ("uv", vp), ("coord_valid", vp), ("out", vp), ("valid", vp),
                ("batch_stride", i64), ("point_stride", i64), ("comp_stride", i64), ("n_points", i64),
                ("B", i32), ("C", i32), ("Hs", i32), ("Ws", i32), ("mode", i32), ("padding", i32), ("normalize", i32), ("src_u8", i32),
                ("out_u8", i32), ("out_rows", i32), ("src_shared", i32), ("mask_shared", i32)]


class UdOverlapMask(C.Structure):
    _fields_ = [("uv", vp), ("mask", vp), ("B", i32), ("H", i32), ("W", i32)]


class UdWarpCamera(C.Structure):
    _fields_ = [("src", vp), ("src_mask", vp), ("src_depth", vp), ("points", vp), ("depth", vp), ("params_dst", vp), ("params_src", vp),
                ("T", vp), ("valid_in", vp), ("out", vp), ("valid", vp), ("visible", vp), ("uv", vp), ("proj_depth", vp),
                ("B", i32), ("C", i32), ("Ho", i32), ("Wo", i32), ("Hs", i32), ("Ws", i32), ("nT", i32), ("mode", i32), ("padding", i32),
                ("normalize", i32), ("src_u8", i32), ("out_u8", i32), ("src_shared", i32), ("mask_shared", i32), ("depth_shared", i32),
                ("tol_bits", i32), ("model_dst", C.c_ubyte * UD_RECON_MAX_B), ("model_src", C.c_ubyte * UD_RECON_MAX_B)]


class UdNormals(C.Structure):
    _fields_ = [("points", vp), ("depth", vp), ("params", vp), ("mask", vp), ("normals", vp), ("valid", vp), ("rgb", vp),
                ("B", i32), ("H", i32), ("W", i32), ("mask_shared", i32), ("has_rtol", i32), ("rtol_bits", i32),
                ("model", C.c_ubyte * UD_RECON_MAX_B)]


class UdDepthConsistency(C.Structure):
    _fields_ = [("depth", vp), ("params_ref", vp), ("valid_in", vp), ("src_depth", vp), ("src_mask", vp), ("params_src", vp), ("T", vp),
                ("Tinv", vp), ("fused", vp), ("count", vp), ("mask", vp), ("consistent", vp), ("err_px", vp), ("err_rel", vp),
                ("B", i32), ("V", i32), ("H", i32), ("W", i32), ("Hs", i32), ("Ws", i32), ("nT", i32), ("min_views", i32),
                ("px_tol_bits", i32), ("rel_tol_bits", i32), ("model_ref", C.c_ubyte * UD_RECON_MAX_B), ("model_src", C.c_ubyte * UD_RECON_MAX_B)]


class UdTsdfIntegrate(C.Structure):
    _fields_ = [("src_depth", vp), ("src_mask", vp), ("src_weight", vp), ("image", vp), ("params", vp), ("T", vp), ("origin", vp),
                ("tsdf", vp), ("weight", vp), ("color", vp), ("count", vp),
                ("B", i32), ("V", i32), ("Nx", i32), ("Ny", i32), ("Nz", i32), ("Hs", i32), ("Ws", i32), ("nT", i32), ("n_origin", i32),
                ("fresh", i32), ("has_max_weight", i32), ("voxel_size_bits", i32), ("trunc_bits", i32), ("max_weight_bits", i32),
                ("model", C.c_ubyte * UD_RECON_MAX_B)]


class UdTsdfPoints(C.Structure):
    _fields_ = [("tsdf", vp), ("weight", vp), ("color", vp), ("origin", vp), ("xyz", vp), ("rgb", vp), ("counts", vp), ("offsets", vp),
                ("work", vp), ("work_bytes", i64), ("capacity", i64),
                ("B", i32), ("Nx", i32), ("Ny", i32), ("Nz", i32), ("n_origin", i32), ("rgb_f32", i32), ("voxel_size_bits", i32),
                ("min_weight_bits", i32)]


class UdTsdfMesh(C.Structure):
    _fields_ = [("tsdf", vp), ("weight", vp), ("color", vp), ("origin", vp), ("vertices", vp), ("rgb", vp), ("normals", vp), ("faces", vp),
                ("vert_counts", vp), ("vert_offsets", vp), ("face_counts", vp), ("face_offsets", vp), ("work", vp), ("work_bytes", i64),
                ("vert_capacity", i64), ("face_capacity", i64),
                ("B", i32), ("Nx", i32), ("Ny", i32), ("Nz", i32), ("n_origin", i32), ("rgb_f32", i32), ("voxel_size_bits", i32),
                ("min_weight_bits", i32)]


class UdTsdfRender(C.Structure):
    _fields_ = [("tsdf", vp), ("weight", vp), ("color", vp), ("origin", vp), ("T", vp), ("params", vp), ("rays", vp),
                ("depth", vp), ("valid", vp), ("points", vp), ("normals", vp), ("color_out", vp),
                ("B", i32), ("Ho", i32), ("Wo", i32), ("Nx", i32), ("Ny", i32), ("Nz", i32), ("nT", i32), ("n_origin", i32), ("K", i32),
                ("color_f32", i32), ("full_scan", i32), ("wave_patch", i32), ("voxel_size_bits", i32), ("near_bits", i32), ("step_bits", i32),
                ("min_weight_bits", i32), ("model", C.c_ubyte * UD_RECON_MAX_B)]


class UdIcp(C.Structure):
    _fields_ = [("depth", vp), ("points", vp), ("params", vp), ("mask", vp), ("weights", vp), ("normals", vp),
                ("model_points", vp), ("model_normals", vp), ("model_valid", vp), ("params_model", vp),
                ("T", vp), ("work", vp), ("system", vp), ("matched", vp), ("residual", vp), ("rows", vp), ("x", vp), ("status", vp), ("stats", vp),
                ("work_bytes", i64), ("stats_stride", i64), ("damping_bits", i64),
                ("B", i32), ("H", i32), ("W", i32), ("Hm", i32), ("Wm", i32), ("nT", i32), ("solve", i32), ("min_count", i32), ("has_cos", i32),
                ("dist_tol_bits", i32), ("cos_tol_bits", i32), ("blocks", i32),
                ("model_frame", C.c_ubyte * UD_RECON_MAX_B), ("model_model", C.c_ubyte * UD_RECON_MAX_B)]


class UdDepthPyramid(C.Structure):
    _fields_ = [("depth", vp), ("mask", vp), ("weights", vp), ("ws", vp), ("wr", vp), ("out_depth", vp * 4), ("out_weights", vp * 4),
                ("B", i32), ("H", i32), ("W", i32), ("levels", i32), ("radius", i32), ("tile", i32), ("gate_bits", i32),
                ("inv_bin_bits", i32)]


UD_EVAL_NORMALS_MAX_T = 8


class UdEvalNormals(C.Structure):
    _fields_ = [("gt", vp), ("pred", vp), ("mask", vp), ("out", vp), ("count", vp), ("error", vp),
                ("B", i32), ("H", i32), ("W", i32), ("T", i32), ("mask_shared", i32), ("cos_bits", i32 * UD_EVAL_NORMALS_MAX_T)]


UD_PC_MINCONF, UD_PC_RANGE, UD_PC_EDGE, UD_PC_FLIP_Y = 1, 2, 4, 8


class UdPointCloud(C.Structure):
    _fields_ = [("points", vp), ("depth", vp), ("K", vp), ("image", vp), ("image_f32", vp), ("mask", vp), ("confidence", vp),
                ("xyz", vp), ("rgb", vp), ("index", vp), ("counts", vp), ("offsets", vp), ("work", vp), ("work_bytes", i64),
                ("capacity", i64), ("B", i32), ("H", i32), ("W", i32), ("nK", i32), ("flags", i32),
                ("min_conf", f32), ("dmin", f32), ("dmax", f32), ("edge_rtol", f32)]


UD_MATCH_MAX_PLANES = 4


class UdMatchPlane(C.Structure):
    _fields_ = [("src", vp), ("mul", vp), ("dst", vp), ("C", i32), ("src_batch_stride", i64)]


class UdMatchGt(C.Structure):
    _fields_ = [("planes", UdMatchPlane * UD_MATCH_MAX_PLANES), ("pads1", vp), ("pads2", vp), ("K_in", vp), ("K_out", vp),
                ("n_planes", i32), ("B", i32), ("h1", i32), ("w1", i32), ("H2", i32), ("W2", i32)]


UD_COLORIZE_MAX_PANELS = 4
UD_CZ_NONE, UD_CZ_MAP, UD_CZ_AREL, UD_CZ_RGB = 0, 1, 2, 3
UD_CZ_AUTO_LO, UD_CZ_AUTO_HI = 1, 2
UD_CZ_CHW = 1


class UdColorPanel(C.Structure):
    _fields_ = [("src", vp), ("src2", vp), ("lut", vp), ("batch_stride", i64), ("batch_stride2", i64), ("kind", i32), ("flags", i32),
                ("lo", f32), ("hi", f32), ("den", f32)]


class UdColorize(C.Structure):
    _fields_ = [("panels", UdColorPanel * UD_COLORIZE_MAX_PANELS), ("dst", vp), ("work", vp), ("work_bytes", i64),
                ("B", i32), ("H", i32), ("W", i32), ("rows", i32), ("cols", i32), ("flags", i32)]


UD_SPLAT_NEAREST, UD_SPLAT_MEAN = 0, 1
UD_SPLAT_TRUNC, UD_SPLAT_RANGE = 1, 2


class UdSplat(C.Structure):
    _fields_ = [("xyz", vp), ("offsets", vp), ("K", vp), ("T", vp), ("color", vp), ("depth", vp), ("index", vp), ("rgb", vp), ("count", vp),
                ("work", vp), ("work_bytes", i64), ("batch_stride", i64), ("point_stride", i64), ("comp_stride", i64), ("n_points", i64),
                ("B", i32), ("H", i32), ("W", i32), ("nK", i32), ("nT", i32), ("mode", i32), ("flags", i32), ("color_f32", i32),
                ("pixel_offset", f32), ("dmin", f32), ("dmax", f32)]


UD_SPLAT_FOV = 4                                      # UdSplatCamera.flags only


class UdSplatCamera(C.Structure):
    _fields_ = [("xyz", vp), ("offsets", vp), ("params", vp), ("T", vp), ("color", vp), ("depth", vp), ("index", vp), ("rgb", vp), ("count", vp),
                ("work", vp), ("work_bytes", i64), ("batch_stride", i64), ("point_stride", i64), ("comp_stride", i64), ("n_points", i64),
                ("B", i32), ("H", i32), ("W", i32), ("nT", i32), ("mode", i32), ("flags", i32), ("color_f32", i32),
                ("pixel_offset", f32), ("dmin", f32), ("dmax", f32), ("cos_limit", f32), ("model", C.c_ubyte * UD_RECON_MAX_B)]


class UdDepthMinPool(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("N", i32), ("H", i32), ("W", i32), ("factor", i32)]


UD_RESIZE_BICUBIC, UD_RESIZE_BILINEAR = 0, 1
UD_RESIZE_OUT_F32, UD_RESIZE_OUT_U8, UD_RESIZE_OUT_NORM = 0, 1, 2
UD_RESIZE_MAX_SCALE, UD_RESIZE_MAX_TAPS = 8, 33


class UdResizeAA(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("mask_src", vp), ("mask_dst", vp), ("K_in", vp), ("K_out", vp),
                ("B", i32), ("C", i32), ("h", i32), ("w", i32), ("top", i32), ("left", i32), ("height", i32), ("width", i32),
                ("Ho", i32), ("Wo", i32), ("dtop", i32), ("dleft", i32), ("Hn", i32), ("Wn", i32),
                ("src_u8", i32), ("filter", i32), ("out_form", i32), ("mean", f32 * 4), ("inv_std", f32 * 4)]


(UD_V1_RESIZE_AA, UD_V1_SH_EMBED, UD_V1_SOFTMAX, UD_V1_ATTN_FEWQ, UD_V1_HEAD_MIX) = range(1, 6)
(UD_V1_ADD, UD_V1_COPY_ROWS) = (8, 9)
(UD_V1_CAMERA, UD_V1_POINTS, UD_V1_MEAN3, UD_V1_PREPROCESS, UD_V1_VIT_TAP) = range(11, 16)
UD_V1_RESIZE_AC_SPLIT = 17
UD_V1_OUT_CONV3 = 18
UD_ACT_CLAMPEXP = 3


class UdAttention(C.Structure):
    _fields_ = [("Q", vp), ("K", vp), ("Vt", vp), ("O", vp), ("B", i32), ("H", i32), ("Nq", i32), ("Nk", i32),
                ("ldq", i32), ("ldk", i32), ("ldo", i32), ("kv_ld", i32), ("q_rows_per_img", i32),
                ("k_rows_per_img", i32), ("scale", f32), ("kv_broadcast", i32), ("kv_group", i32), ("q_prescaled", i32)]


class UdPreprocess(C.Structure):
    _fields_ = [("rgb", vp), ("patches", vp), ("B", i32), ("H", i32), ("W", i32), ("pad_l", i32), ("pad_t", i32),
                ("Hp", i32), ("Wp", i32), ("Hn", i32), ("Wn", i32), ("ldp", i32), ("is_u8", i32), ("normalize", i32),
                ("mean", f32 * 3), ("inv_std", f32 * 3)]


class UdRayEmbed(C.Structure):
    _fields_ = [("rays", fp), ("scales", fp), ("xhat", vp), ("nb", i32), ("Hn", i32), ("Wn", i32), ("h", i32),
                ("w", i32), ("C", i32), ("ldy", i32), ("rows_per_img", i32), ("eps", f32)]


class UdUpsample2x(C.Structure):
    _fields_ = [("in_", vp), ("out", vp), ("B", i32), ("H", i32), ("W", i32), ("C", i32), ("ldin", i32), ("ldy", i32),
                ("mode", i32), ("eps", f32), ("in_img_rows", i32)]


class UdResizeAC(C.Structure):
    _fields_ = [("in_", vp), ("out", vp), ("G", i32), ("B", i32), ("Hin", i32), ("Win", i32), ("Hout", i32),
                ("Wout", i32), ("C", i32)]


class UdFinalize(C.Structure):
    _fields_ = [("radius_net", fp), ("conf_net", fp), ("rays_net", fp), ("confidence", fp), ("radius", fp),
                ("depth", fp), ("points", fp), ("rays", fp), ("B", i32), ("nb_rays", i32), ("Hn", i32), ("Wn", i32),
                ("Hp", i32), ("Wp", i32), ("pad_l", i32), ("pad_t", i32), ("Ho", i32), ("Wo", i32), ("mode", i32)]


P = C.POINTER
# argument types of every function include/unidepth_hip.h declares; the return type is i32 unless RESTYPE says otherwise
SIG = {
    "ud_gemm_f16": [P(UdGemm), vp],
    "ud_gemm_pick": [P(UdGemm)],
    "ud_gemm_kernel_name": [P(UdGemm), C.c_char_p, i32],
    "ud_layernorm_f32_f16": [P(UdLayerNorm), vp],
    "ud_rccl_unique_id": [vp],
    "ud_rccl_init": [vp, i32, i32],
    "ud_rccl_allgather_outputs": [vp, vp, C.c_size_t, i32, vp],
    "ud_rccl_finalize": [],
    "ud_attention_f16": [P(UdAttention), vp],
    "ud_row_stats_finalize": [vp, vp, i32, i32, i32, f32, vp],
    "ud_program_add_row_stats_finalize": [vp, vp, vp, i32, i32, i32, f32],
    "ud_linear_f32": [P(UdLinearF32), vp],
    "ud_attention_small_f32": [vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "ud_program_add_linear_f32": [vp, P(UdLinearF32)],
    "ud_camera_head_f32": [P(UdCameraHead), vp],
    "ud_camera_head_supported": [P(UdCameraHead)],
    "ud_program_add_camera_head": [vp, P(UdCameraHead)],
    "ud_program_add_attention_small_f32": [vp, vp, vp, vp, i32, i32, i32, i32, f32],
    "ud_preprocess_patches": [P(UdPreprocess), vp],
    "ud_fill_rows_f32": [vp, vp, i32, i32, i32, i32, i32, vp],
    "ud_camera_intrinsics": [vp, i32, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, vp],
    "ud_rays_from_kinv": [vp, vp, i32, i32, i32, i32, vp],
    "ud_rays_from_camera": [vp, vp, vp, i32, i32, i32, vp],
    "ud_ray_embed": [P(UdRayEmbed), vp],
    "ud_upsample2x_nhwc": [P(UdUpsample2x), vp],
    "ud_resize_ac_nhwc_f16": [P(UdResizeAC), vp],
    "ud_finalize_outputs": [P(UdFinalize), vp],
    "ud_nhwc_to_nchw_f32": [vp, vp, i32, i32, i32, i32, i32, vp],
    "ud_program_destroy": [vp],
    "ud_program_size": [vp],
    "ud_program_add_gemm": [vp, P(UdGemm)],
    "ud_program_add_layernorm": [vp, P(UdLayerNorm)],
    "ud_program_add_attention": [vp, P(UdAttention)],
    "ud_program_add_preprocess": [vp, P(UdPreprocess)],
    "ud_program_add_fill_rows": [vp, vp, vp, i32, i32, i32, i32, i32],
    "ud_program_add_camera_intrinsics": [vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32],
    "ud_program_add_rays": [vp, vp, vp, i32, i32, i32, i32],
    "ud_program_add_rays_camera": [vp, vp, vp, vp, i32, i32, i32],
    "ud_program_add_ray_embed": [vp, P(UdRayEmbed)],
    "ud_program_add_upsample2x": [vp, P(UdUpsample2x)],
    "ud_program_add_resize_ac": [vp, P(UdResizeAC)],
    "ud_program_add_finalize": [vp, P(UdFinalize)],
    "ud_program_add_nhwc_to_nchw": [vp, vp, vp, i32, i32, i32, i32, i32],
    "ud_dwconv7_nhwc_f32": [P(UdDwConv7), vp],
    "ud_layernorm_patchify2": [vp, vp, i32, i32, i32, i32, i32, f32, vp],
    "ud_patchify4_nchw": [vp, vp, i32, i32, i32, i32, vp],
    "ud_max_f32": [vp, vp, i64, i32, vp],
    "ud_spatial_mean_f32": [vp, vp, i32, i32, i32, i32, vp],
    "ud_program_add_dwconv7": [vp, P(UdDwConv7)],
    "ud_program_add_layernorm_patchify2": [vp, vp, vp, i32, i32, i32, i32, i32, f32],
    "ud_program_add_patchify4": [vp, vp, vp, i32, i32, i32, i32],
    "ud_program_add_max": [vp, vp, vp, i64, i32],
    "ud_program_add_spatial_mean": [vp, vp, vp, i32, i32, i32, i32],
    "ud_v1_op": [P(UdV1Op), vp],
    "ud_program_add_v1_op": [vp, P(UdV1Op)],
    "ud_knn_points": [P(UdKnn), vp],
    "ud_knn_split": [P(UdKnn)],
    "ud_extract_patches": [P(UdExtractPatches), vp],
    "ud_eval_depth": [P(UdEvalDepth), vp],
    "ud_eval_3d": [P(UdEval3d), vp],
    "ud_reconstruct": [P(UdReconstruct), vp],
    "ud_pointcloud_pack": [P(UdPointCloud), vp],
    "ud_match_gt": [P(UdMatchGt), vp],
    "ud_colorize": [P(UdColorize), vp],
    "ud_splat": [P(UdSplat), vp],
    "ud_splat_camera": [P(UdSplatCamera), vp],
    "ud_camera_project": [P(UdCameraProject), vp],
    "ud_camera_unproject": [P(UdCameraUnproject), vp],
    "ud_remap": [P(UdRemap), vp],
    "ud_overlap_mask": [P(UdOverlapMask), vp],
    "ud_warp_camera": [P(UdWarpCamera), vp],
    "ud_normals": [P(UdNormals), vp],
    "ud_depth_consistency": [P(UdDepthConsistency), vp],
    "ud_tsdf_integrate": [P(UdTsdfIntegrate), vp],
    "ud_tsdf_points": [P(UdTsdfPoints), vp],
    "ud_tsdf_render": [P(UdTsdfRender), vp],
    "ud_tsdf_mesh": [P(UdTsdfMesh), vp],
    "ud_icp_linearize": [P(UdIcp), vp],
    "ud_icp_update": [P(UdIcp), vp],
    "ud_depth_pyramid": [P(UdDepthPyramid), vp],
    "ud_eval_normals": [P(UdEvalNormals), vp, i64, vp],
    "ud_depth_minpool": [P(UdDepthMinPool), vp],
    "ud_resize_aa": [P(UdResizeAA), vp],
    "ud_program_run": [vp, i32, i32, vp],
    "ud_calib_mfma_stream": [vp, i32, i32, vp, P(C.c_double), vp],
    "ud_calib_mfma_stream16": [vp, i32, i32, vp, P(C.c_double), vp],
    "ud_version": [],
    "ud_struct_size": [i32],
    "ud_eval_depth_work_bytes": [i32, i32, i32],
    "ud_eval_3d_work_bytes": [i32, i32, i32, i32],
    "ud_eval_normals_work_bytes": [i32, i32, i32, i32],
    "ud_reconstruct_work_bytes": [i32, i32, i32, i32],
    "ud_camera_unproject_work_bytes": [i32, i32],
    "ud_pointcloud_work_bytes": [i32, i32, i32],
    "ud_tsdf_points_work_bytes": [i32, i32, i32, i32],
    "ud_tsdf_mesh_work_bytes": [i32, i32, i32, i32],
    "ud_icp_workspace_bytes": [i32, i32, i32],
    "ud_colorize_work_bytes": [i32, i32, i32],
    "ud_splat_work_bytes": [i32, i32, i32],
    "ud_program_create": [],
    "ud_last_error": [],
}
RESTYPE = {"ud_program_destroy": None, "ud_program_create": vp, "ud_last_error": C.c_char_p}
RESTYPE.update(dict.fromkeys((
    "ud_eval_depth_work_bytes", "ud_eval_3d_work_bytes", "ud_eval_normals_work_bytes", "ud_reconstruct_work_bytes",
    "ud_camera_unproject_work_bytes", "ud_pointcloud_work_bytes", "ud_tsdf_points_work_bytes", "ud_tsdf_mesh_work_bytes",
    "ud_icp_workspace_bytes", "ud_colorize_work_bytes", "ud_splat_work_bytes"), i64))

# ud_struct_size(i) of the library; the numbers missing here are not assigned: the library answers -1
STRUCT_INDEX = {
    0: UdGemm, 1: UdLayerNorm, 2: UdAttention, 3: UdPreprocess, 4: UdRayEmbed, 5: UdUpsample2x, 6: UdResizeAC, 7: UdFinalize, 8: UdLinearF32,
    9: UdDwConv7, 10: UdV1Op, 11: UdKnn, 12: UdExtractPatches, 13: UdCameraHead, 14: UdEvalDepth, 15: UdPointCloud, 17: UdMatchGt, 18: UdColorize,
    20: UdSplat, 21: UdDepthMinPool, 23: UdResizeAA, 25: UdEval3d, 27: UdReconstruct, 28: UdCameraProject, 29: UdSplatCamera, 31: UdCameraUnproject,
    33: UdRemap, 34: UdOverlapMask, 36: UdWarpCamera, 38: UdNormals, 39: UdEvalNormals, 41: UdDepthConsistency, 43: UdTsdfIntegrate, 44: UdTsdfPoints,
    45: UdTsdfRender, 46: UdTsdfMesh, 48: UdIcp, 49: UdDepthPyramid,
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP kernel library is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or unidepth_amd/csrc/build.sh (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, args in SIG.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = RESTYPE.get(name, i32)
    for i, st in STRUCT_INDEX.items():
        # a library whose descriptors differ from this mirror in ANY way is a hard error (A/B runs rebuild both arms from one tree:
        # an older .so would read the appended fields -- a_wrap, row_stats_* -- as garbage or not at all)
        if lib.ud_struct_size(i) != C.sizeof(st):
            raise ImportError(f"ctypes mirror of {st.__name__} is out of sync with include/unidepth_hip.h "
                              f"({C.sizeof(st)} vs {lib.ud_struct_size(i)} bytes)")
    return lib


lib = _load()


def check(rc: int, what: str = ""):
    if rc < 0:
        raise RuntimeError(f"unidepth_hip {what} failed (code {rc}): {lib.ud_last_error().decode()}")
    return rc
