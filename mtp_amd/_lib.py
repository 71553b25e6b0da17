"""ctypes binding of libmtp_hip.so (the C ABI declared in include/mtp_hip.h).

The product path has NO fallback: if the library is missing or a symbol does not resolve, importing the
ops raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or `make -C mtp_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTP_HIP_LIB") or os.path.join(_HERE, "libmtp_hip.so")   # MTP_HIP_LIB: A/B builds of the same ABI

MTP_F32, MTP_BF16, MTP_F64 = 0, 1, 2      # (MTP_F64: the DCNv3 entry points only)
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_DGELU, EPI_BIAS_GELU_DG, EPI_MUL = 0, 1, 2, 3, 4, 5

# enum mtp_gemm_variant (GemmArgs.variant), same names without the MTP_ prefix; tests/test_abi.py checks them against the header
GEMM_NT_REG_STAGED = 1
GEMM_ORDER_SHIFT, GEMM_ORDER_PLAIN, GEMM_ORDER_GROUPED, GEMM_ORDER_ROW_MAJOR, GEMM_ORDER_MASK = 1, 1 << 1, 2 << 1, 3 << 1, 3 << 1
GEMM_TNG_PLAIN_ORDER = 1 << 1
GEMM_TN_REG_TRANSPOSE = 1 << 4
GEMM_NT_SB8, GEMM_NT_NO_SB8 = 1 << 5, 1 << 6
GEMM_NT_P8, GEMM_NT_P8_224, GEMM_NT_P8_256, GEMM_NT_P8_MASK, GEMM_NT_NO_P8 = 1 << 8, 2 << 8, 3 << 8, 3 << 8, 1 << 10
GEMM_NT_PERSIST, GEMM_TN_TR_FULL_ONLY, GEMM_NT_NO_PERSIST = 1 << 15, 1 << 15, 1 << 16
GEMM_NT_STRIP, GEMM_NT_NO_STRIP = 1 << 17, 1 << 18
GEMM_TNG_PLAIN_PHASES = 1 << 19
GEMM_STORE_SHIFT, GEMM_STORE_NT, GEMM_STORE_SC1, GEMM_STORE_PLAIN, GEMM_STORE_MASK = 20, 1 << 20, 2 << 20, 3 << 20, 3 << 20
# enum mtp_gemm_nt_family (GemmNtPlan.family)
GEMM_NT_FAMILY_SB, GEMM_NT_FAMILY_SB8, GEMM_NT_FAMILY_REG, GEMM_NT_FAMILY_P8, GEMM_NT_FAMILY_STRIP = 0, 1, 2, 3, 4

# enum mtp_conv_op / mtp_conv_kernel_family (mtp_conv_kernel) and mtp_dcnv3_kernel_family (mtp_dcnv3_kernel)
CONV_OP_IM2COL3X3, CONV_OP_COL2IM3X3, CONV_OP_DWCONV3X3_FWD, CONV_OP_DWCONV3X3_BWD_DX, CONV_OP_DWCONV3X3_BWD_DW = 0, 1, 2, 3, 4
CONV_KERNEL_NONE, CONV_KERNEL_ELEMENT, CONV_KERNEL_V8, CONV_KERNEL_P8, CONV_KERNEL_PX4 = 0, 1, 2, 3, 4
DCNV3_KERNEL_NONE, DCNV3_FWD9, DCNV3_FWD_VEC8, DCNV3_FWD_SCALAR, DCNV3_F64 = 0, 1, 2, 3, 4
DCNV3_BWD_WINDOW_R2, DCNV3_BWD_WINDOW_R3, DCNV3_BWD_3X3_OS1, DCNV3_BWD_3X3_OS2, DCNV3_BWD_SCATTER_SHFL, DCNV3_BWD_SCATTER_ATOMIC = 5, 6, 7, 8, 9, 10

# enum mtp_box_kind / mtp_assign_calculator (csrc/box_ops.hip)
BOX_ALIGNED, BOX_ROTATED = 0, 1
ASSIGN_BOX, ASSIGN_RBOX2HBOX, ASSIGN_ROTATED = 0, 1, 2
# csrc/det_eval.hip: MTP_DET_MAX_THRS / MTP_DET_MAX_CLASSES / MTP_DET_AP_POINTS and enum mtp_det_ap_mode
DET_MAX_THRS, DET_MAX_CLASSES, DET_AP_POINTS = 8, 4096, 11
DET_AP_11POINTS, DET_AP_AREA = 0, 1
# csrc/coco_eval.hip: MTP_COCO_MAX_THRS / _AREAS / _MAX_DET_LEVELS / _MAX_CLASSES / _REC_THRS / _MAX_CELL_GTS and enum mtp_coco_kind
COCO_MAX_THRS, COCO_AREAS, COCO_MAX_DET_LEVELS, COCO_MAX_CLASSES, COCO_REC_THRS, COCO_MAX_CELL_GTS = 16, 4, 4, 4096, 101, 4096
COCO_BBOX, COCO_SEGM = 0, 1

# enum mtp_hroi_target (mtp_hroi_loss, csrc/hbox_head.hip)
HROI_TARGET_ONES, HROI_TARGET_ENCODED = 0, 1

# enum mtp_fuse_policy (mtp_fuse_pair_fwd / _bwd)
FUSE_CONCAT, FUSE_SUM, FUSE_DIFF, FUSE_ABS_DIFF = 0, 1, 2, 3

p, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float


class GemmArgs(C.Structure):
    _fields_ = [("A", p), ("B", p), ("C", p), ("M", i64), ("N", i64), ("K", i64),
                ("lda", i64), ("ldb", i64), ("ldc", i64),
                ("in_dtype", i32), ("out_dtype", i32), ("epilogue", i32),
                ("bias", p), ("bias_mod", i64), ("res", p), ("res_ld", i64), ("res_mod", i64),
                ("rowscale", p), ("rows_per_sample", i64), ("aux", p), ("aux_ld", i64),
                ("split_k", i32), ("variant", i32), ("colsum", p), ("defer_sum", i32), ("pad_", i32),
                ("workspace", p), ("workspace_bytes", i64)]


class GemmNtPlan(C.Structure):
    """struct mtp_gemm_nt_plan"""
    _fields_ = [("family", i32), ("tile_m", i32), ("order", i32), ("persistent", i32), ("store_policy", i32)]


# kinds of struct mtp_nt_rider (mtp_gemm_nt_rider)
NT_RIDER_NONE, NT_RIDER_SAMPLING_FWD, NT_RIDER_SAMPLING_BWD_WIN = 0, 1, 2


class NtRider(C.Structure):
    """struct mtp_nt_rider"""
    _fields_ = [("kind", i32), ("act_dtype", i32), ("x", p), ("dsamp", p), ("w", p), ("bias", p), ("avg", p), ("pooled", p), ("samp", p), ("g", p),
                ("B", i64), ("Hp", i64), ("Wp", i64), ("windows", i64), ("C", i64), ("N", i64)]


# reasons of struct mtp_nt_rider_plan (mtp_gemm_nt_rider_plan)
NT_RIDE_OK, NT_RIDE_NO_FAMILY, NT_RIDE_NO_INSTANTIATION, NT_RIDE_NO_SPARE_CU, NT_RIDE_NO_SCRATCH = 0, 1, 2, 3, 4


class NtRiderPlan(C.Structure):
    """struct mtp_nt_rider_plan"""
    _fields_ = [("rides", i32), ("gemm_wgs", i32), ("riders", i32), ("windows_per_rider", i32), ("scratch_bytes", i32), ("reason", i32)]


class WimgDesc(C.Structure):
    """mtp_wimg_desc"""
    _fields_ = [("src", p), ("w", p), ("wt", p), ("R", i64), ("C", i64), ("tile0", i64), ("f32_out", C.c_int32), ("wd", C.c_float)]


class Dcnv3Geom(C.Structure):
    """mtp_dcnv3_geom"""
    _fields_ = [("N", i64), ("H", i64), ("W", i64), ("kernel_h", C.c_int32), ("kernel_w", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32),
                ("pad_h", C.c_int32), ("pad_w", C.c_int32), ("dilation_h", C.c_int32), ("dilation_w", C.c_int32), ("group", C.c_int32),
                ("group_channels", C.c_int32), ("offset_scale", C.c_float), ("im2col_step", C.c_int32), ("remove_center", C.c_int32), ("variant", C.c_int32)]


RPN_MAX_LEVELS = 8


class RpnLevel(C.Structure):
    """struct mtp_rpn_level"""
    _fields_ = [("cls", p), ("reg", p), ("dcls", p), ("dreg", p), ("H", i64), ("W", i64), ("keep_count", i64), ("cls_stride", i64 * 4), ("reg_stride", i64 * 4)]


ROI_MAX_LEVELS = 8


class RoiLevel(C.Structure):
    """struct mtp_roi_level"""
    _fields_ = [("map", p), ("dmap", p), ("H", i64), ("W", i64), ("spatial_scale", f32), ("stride", i64 * 4)]


# name -> (restype, argtypes); must list EVERY function declared in include/mtp_hip.h (tests/test_abi.py checks)
SIGNATURES = {
    "mtp_weight_images": (i32, [p, i32, i64, i32, p]),
    "mtp_dwconv_fwd": (i32, [p, p, p, p, i32, i64, i64, i64, i64, i32, p]),
    "mtp_dwconv_bwd_dx": (i32, [p, i32, p, p, i32, i64, i64, i64, i64, i32, p]),
    "mtp_dwconv_bwd_dw": (i32, [p, p, i32, p, p, i64, i64, i64, i64, i32, p]),
    "mtp_center_feature_scale_fwd": (i32, [p, p, p, i64, p, i32, i64, i64, i64, p]),
    "mtp_center_feature_scale_bwd": (i32, [p, p, p, p, i64, p, p, p, i32, i64, i64, i64, p]),
    "mtp_dcnv3_out_size": (i32, [C.POINTER(Dcnv3Geom), C.POINTER(i64), C.POINTER(i64)]),
    "mtp_dcnv3_fwd": (i32, [p, p, p, p, i32, C.POINTER(Dcnv3Geom), p]),
    "mtp_dcnv3_bwd": (i32, [p, p, p, p, i32, p, p, p, C.POINTER(Dcnv3Geom), p]),
    "mtp_dcnv3_bwd_act": (i32, [p, p, p, p, i32, p, p, p, p, i64, C.POINTER(Dcnv3Geom), p]),
    "mtp_dcnv3_kernel": (i32, [p, p, p, p, p, p, p, i32, C.POINTER(Dcnv3Geom), i32]),
    "mtp_conv_kernel": (i32, [i32, p, i32, i64, i64, i64, i64, p, i32, p, p, i64, i64, i64, i64, i64, i64]),
    "mtp_gemm_nt": (i32, [C.POINTER(GemmArgs), p]),
    "mtp_gemm_nt_plan": (i32, [C.POINTER(GemmArgs), i32, C.POINTER(GemmNtPlan)]),
    "mtp_gemm_nt_tile": (i32, [C.POINTER(GemmArgs)]),
    "mtp_gemm_nt_workspace_bytes": (i64, []),
    "mtp_gemm_nt_rider": (i32, [C.POINTER(GemmArgs), C.POINTER(NtRider), p]),
    "mtp_gemm_nt_rider_plan": (i32, [C.POINTER(GemmArgs), C.POINTER(NtRider), i32, C.POINTER(NtRiderPlan)]),
    "mtp_nt_p8_gemm_wgs": (i32, [i32, i32]),
    "mtp_gemm_tn": (i32, [C.POINTER(GemmArgs), p]),
    "mtp_gemm_tn_grouped": (i32, [C.POINTER(GemmArgs), i32, p]),
    "mtp_sum_partials_batch": (i32, [p, p, p, p, i32, p]),
    "mtp_layernorm_fwd": (i32, [p, i32, p, p, p, i32, p, p, i64, i64, f32, i32, p]),
    "mtp_layernorm_bwd_partial_rows": (i64, [i64]),
    "mtp_layernorm_bwd": (i32, [p, i32, p, i32, p, p, p, p, i32, p, p, p, i32, p, i32, p, i64, p, p, i64, i64, i64, p]),
    "mtp_reduce_rows_f32": (i32, [p, i64, p, i64, i64, i32, p]),
    "mtp_reduce_rows_batched_f32": (i32, [p, p, i32, i64, i64, i64, i32, p]),
    "mtp_reduce_rows_t_f32": (i32, [p, i64, p, i64, i64, i64, i32, p]),
    "mtp_reduce_rows_t_batched_f32": (i32, [p, p, i32, i64, i64, i64, i64, i32, p]),
    "mtp_copy_segments_f32": (i32, [p, p, p, i32, p]),
    "mtp_colsum": (i32, [p, i32, i64, p, i64, i64, p]),
    "mtp_colsum_acc": (i32, [p, i32, i64, p, i64, i64, p]),
    "mtp_patchify": (i32, [p, p, i32, i64, i64, i64, i64, i64, p]),
    "mtp_preprocess_patchify": (i32, [p, p, i32, i64, i64, i64, i64, i64, C.POINTER(f32), C.POINTER(f32), i32, f32, p]),
    "mtp_unpatchify": (i32, [p, i32, p, i64, i64, i64, i64, i64, p]),
    "mtp_cast": (i32, [p, i32, p, i32, i64, p]),
    "mtp_transpose_cast": (i32, [p, p, i32, i64, i64, p]),
    "mtp_convt_pack": (i32, [p, p, p, i32, i64, i64, p]),
    "mtp_convt_unpack_grad": (i32, [p, p, i64, i64, p]),
    "mtp_tokens_to_nchw": (i32, [p, i32, p, i32, i64, i64, i64, i64, i32, p]),
    "mtp_nchw_to_tokens": (i32, [p, i32, p, i32, i64, i64, i64, i64, i32, p]),
    "mtp_maxpool2_tokens_fwd": (i32, [p, p, i32, i64, i64, i64, i64, p]),
    "mtp_maxpool2_tokens_bwd": (i32, [p, p, i32, p, i32, i64, i64, i64, i64, p]),
    "mtp_axpy_f32": (i32, [p, p, f32, i64, p]),
    "mtp_scale_rows_cast": (i32, [p, p, i32, p, i64, i64, i64, p]),
    "mtp_im2col3x3": (i32, [p, i32, i64, i64, i64, i64, p, i32, i64, i64, i64, i64, i64, i64, p]),
    "mtp_col2im3x3": (i32, [p, i32, p, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i32, p]),
    "mtp_conv3x3_pack": (i32, [p, p, p, i32, i64, i64, i64, p]),
    "mtp_conv3x3_unpack_grad": (i32, [p, p, i64, i64, i64, p]),
    "mtp_pack_rows_padded": (i32, [p, p, p, i32, i64, i64, i64, p]),
    "mtp_cast_pad_rows": (i32, [p, i64, p, i32, i64, i64, p]),
    "mtp_copy_rows": (i32, [p, i64, p, i64, i32, i64, i64, p]),
    "mtp_dwconv3x3_fwd": (i32, [p, p, p, p, i32, i64, i64, i64, i64, p]),
    "mtp_dwconv3x3_bwd_dx": (i32, [p, i32, p, p, i32, i64, i64, i64, i64, p]),
    "mtp_dwconv3x3_bwd_dw_partial_rows": (i64, [i64, i64, i64]),
    "mtp_dwconv3x3_bwd_dw": (i32, [p, p, i32, p, i64, i64, i64, i64, p]),
    "mtp_softmax_groups_fwd": (i32, [p, i64, p, i32, i64, i64, i64, p]),
    "mtp_softmax_groups_bwd": (i32, [p, p, p, i64, i32, i64, i64, i64, p]),
    "mtp_scale_residual_fwd": (i32, [p, p, i32, p, p, i64, p, p, i64, i64, p]),
    "mtp_scale_residual_bwd_partial_rows": (i64, [i64]),
    "mtp_scale_residual_bwd": (i32, [p, p, i32, p, p, i64, p, p, i64, i64, p]),
    "mtp_comm_unique_id": (i32, [p]),
    "mtp_comm_init": (i32, [p, i32, i32, C.POINTER(C.c_void_p)]),
    "mtp_comm_allreduce_bucket": (i32, [p, p, i64, p]),
    "mtp_comm_allreduce_bucket_dt": (i32, [p, p, i64, i32, p]),
    "mtp_comm_reduce_scatter_bucket": (i32, [p, p, i64, i32, i32, p]),
    "mtp_comm_allgather_bucket": (i32, [p, p, i64, i32, i32, p]),
    "mtp_comm_info": (i32, [p, p]),
    "mtp_comm_destroy": (i32, [p]),
    "mtp_full_attn_fwd": (i32, [p, p, p, i32, p, p, i64, i64, i64, i64, i64, f32, p]),
    "mtp_full_attn_bwd_workspace_floats": (i64, [i64, i64, i64, i64]),
    "mtp_full_attn_bwd": (i32, [p, p, p, p, p, i32, p, p, p, p, i64, i64, i64, i64, i64, f32, p]),
    "mtp_full_attn_kernel": (i32, [i32, i64, i64, i32]),
    "mtp_rvsa_attn_kernel": (i32, [i32, i64, i64, i64, i32]),
    "mtp_rvsa_pool_fwd": (i32, [p, i32, p, p, i64, i64, i64, i64, p]),
    "mtp_rvsa_pool_bwd": (i32, [p, p, p, i32, i32, i64, i64, i64, i64, p]),
    "mtp_rvsa_sampling_fwd": (i32, [p, i32, p, p, p, p, p, i64, i64, i64, i64, i64, p]),
    "mtp_rvsa_sampling_bwd": (i32, [p, p, p, p, i32, i64, i64, i64, i64, i64, p]),
    "mtp_rvsa_sampling_bwd_win": (i32, [p, p, p, p, i64, i64, i64, p]),
    "mtp_layernorm_residual_fwd": (i32, [p, i32, p, p, p, p, p, i64, p, p, p, p, i64, i64, f32, p]),
    "mtp_layernorm_residual_bwd": (i32, [p, p, i32, p, p, p, p, p, p, i64, p, p, i64, i64, p]),
    "mtp_layernorm_bwd_win": (i32, [p, i32, p, i32, p, p, p, p, p, p, i32, p, i32, p, i64, p, p, i64, i64, i64, p, i64, i64, i64, p]),
    "mtp_small_linear_fwd": (i32, [p, p, p, p, i64, i64, i64, p]),
    "mtp_small_linear_bwd": (i32, [p, p, p, p, p, p, i64, i64, i64, p]),
    "mtp_small_linear_dw_segments": (i32, [p, p, i64, i64, i64, i32, p, p, p, p]),
    "mtp_small_linear_dw_segments_batched": (i32, [p, p, i32, i64, i64, i64, i32, p, p, p, p]),
    "mtp_rvsa_attn_fwd": (i32, [p, p, p, p, i32, p, p, p, i64, i64, i64, i64, i64, f32, p]),
    "mtp_rvsa_attn_bwd": (i32, [p, p, p, p, p, p, p, p, p, p, i32, p, p, p, i64, i64, i64, i64, i64, f32, p]),
    "mtp_zero_segments_f32": (i32, [p, p, p, i32, p]),
    "mtp_sqnorm_f32": (i32, [p, p, i64, p]),
    "mtp_sqnorm_segments_f32": (i32, [p, p, p, i32, p, p]),
    "mtp_adamw_flat": (i32, [p, p, p, p, i64, p, p, i32, p, p, f32, f32, p]),
    "mtp_adamw_weight_images": (i32, [p, i32, i64, i32, p, p, p, p, p, p, f32, f32, p]),
    "mtp_adamw_flat_lr": (i32, [p, p, p, p, i64, p, p, p, i32, p, p, f32, f32, p]),
    "mtp_adamw_weight_images_lr": (i32, [p, p, i32, i64, i32, p, p, p, p, p, p, f32, f32, p]),
    "mtp_bn_partial_rows": (i64, [i64]),
    "mtp_bn_stats": (i32, [p, i32, i64, p, p, p, i64, i64, p]),
    "mtp_bn_finalize": (i32, [p, p, C.c_double, p, p, f32, f32, p, p, i64, p]),
    "mtp_bn_apply": (i32, [p, i32, i64, p, p, p, p, i32, p, i32, i64, i64, i64, p]),
    "mtp_bn_bwd_stats": (i32, [p, i32, i64, p, i32, i64, p, p, p, p, i32, p, p, i64, i64, p]),
    "mtp_bn_bwd_dx": (i32, [p, i32, i64, p, i32, i64, p, p, p, p, i32, p, C.c_double, p, i32, i64, i64, i64, p]),
    "mtp_resize_bilinear_fwd": (i32, [p, i32, i64, p, i32, i64, i64, i64, i64, i64, i64, i64, i32, p]),
    "mtp_resize_bilinear_bwd": (i32, [p, i32, i64, p, i64, i64, i64, i64, i64, i64, i64, i32, p]),
    "mtp_adaptive_avg_pool_fwd": (i32, [p, i32, i64, p, i32, i64, i64, i64, i64, i64, p]),
    "mtp_adaptive_avg_pool_bwd": (i32, [p, i32, p, i64, i64, i64, i64, i64, i64, i32, p]),
    "mtp_channel_scale": (i32, [p, i32, i64, p, i64, p, i32, i64, i64, i64, p]),
    "mtp_seg_ce_workspace_bytes": (i64, [i64, i64, i64, i64]),
    "mtp_seg_ce": (i32, [p, i32, i64, i64, i64, i64, i64, p, i32, i64, i64, i32, f32, p, p, i64, p, i64, p]),
    "mtp_seg_window_accumulate": (i32, [p, i32, i64, i64, i64, i64, i64, p, i64, i64, i64, i64, i64, i64, i64, p]),
    "mtp_seg_argmax_areas": (i32, [p, i64, i64, i64, i64, i64, p, p, i32, p, p, p, i32, i32, p, p]),
    "mtp_seg_areas": (i32, [p, i32, p, i32, i64, i64, i32, p, p]),
    "mtp_fuse_pair_fwd": (i32, [p, i32, p, i32, i64, i64, i64, i64, i64, i32, p]),
    "mtp_fuse_pair_bwd": (i32, [p, i64, p, i32, p, i64, i64, i64, i64, i32, p]),
    "mtp_unet_up_cat_fwd": (i32, [p, i64, i64, p, i64, i64, i32, p, i32, i64, i64, i64, i64, i64, i64, p]),
    "mtp_unet_up_cat_bwd": (i32, [p, i64, p, i64, i64, p, i64, i64, i64, i64, i64, i64, i64, i32, p]),
    "mtp_gap_fwd": (i32, [p, i32, p, i64, i64, i64, p]),
    "mtp_gap_bwd": (i32, [p, p, i32, i64, i64, i64, p]),
    "mtp_cls_ce": (i32, [p, p, p, p, f32, p, p, p, p, p, p, p, i64, i64, i64, p]),
    "mtp_cls_head_bwd": (i32, [p, p, p, p, p, p, i64, i64, i64, i32, p]),
    "mtp_cls_hits": (i32, [p, p, i64, i64, C.POINTER(C.c_int32), i32, f32, i32, p, p]),
    "mtp_box_iou": (i32, [p, p, p, i64, i64, i32, i32, i32, f32, p]),
    "mtp_nms_mask": (i32, [p, p, i64, i32, f32, p, i64, p]),
    "mtp_nms_scan": (i32, [p, i64, i64, p, p, p]),
    "mtp_max_iou_assign": (i32, [p, p, p, i64, i64, i32, f32, f32, f32, f32, i32, i32, p, p, p, p, i64, p]),
    "mtp_det_match": (i32, [p, p, p, p, i64, p, p, p, p, i64, i64, C.POINTER(f32), i32, p, p, p, i64, p]),
    "mtp_det_tpfp": (i32, [p, p, p, i64, p, p, i64, C.POINTER(f32), i32, p, i64, p, p, p]),
    "mtp_det_ap": (i32, [p, p, p, p, i64, i64, i32, i32, C.POINTER(C.c_double), p, p, p, p, p, p]),
    "mtp_mask_pack": (i32, [p, i64, i64, p, p, p]),
    "mtp_coco_iou": (i32, [i32, p, p, p, p, i64, p, p, p, p, p, i64, i64, i32, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), p, p, i64, p]),
    "mtp_coco_match": (i32, [p, i64, p, p, p, i64, p, p, p, p, p, i64, i64, i64, C.POINTER(C.c_double), i32, C.POINTER(C.c_double), i32, p, p, p, p, p]),
    "mtp_coco_accumulate": (i32, [p, p, p, p, p, p, p, i64, i64, i32, C.POINTER(i32), i32, C.POINTER(C.c_double), p, p, p, p]),
    "mtp_rpn_anchors": (i32, [p, i64, i64, i64, i64, i64, i64, i64, i64, i64, f32, p, p, p]),
    "mtp_rpn_loss_workspace_bytes": (i64, [i64, i64]),
    "mtp_rpn_loss": (i32, [C.POINTER(RpnLevel), i32, i64, p, i64, p, i64, p, p, p, p, i64, i64, C.POINTER(f32), C.POINTER(f32), f32, f32, f32, p, p, p, i64, p]),
    "mtp_rpn_proposals": (i32, [C.POINTER(RpnLevel), i32, i64, p, i64, p, i64, C.POINTER(f32), C.POINTER(f32), f32, p, p, p, p, p, p]),
    "mtp_rpn_encode": (i32, [p, p, C.POINTER(f32), C.POINTER(f32), i64, p, p]),
    "mtp_rpn_decode": (i32, [p, p, C.POINTER(f32), C.POINTER(f32), i64, p, p]),
    "mtp_roi_align_rotated_fwd": (i32, [C.POINTER(RoiLevel), i32, i64, i64, p, p, p, i64, i64, i32, i32, i32, f32, p, p, p]),
    "mtp_roi_align_rotated_entries": (i64, [i64, i32, i32]),
    "mtp_roi_align_rotated_bwd_entries": (i32, [C.POINTER(RoiLevel), i32, i64, p, p, p, i64, i64, i32, i32, i32, f32, p, p, p]),
    "mtp_roi_align_rotated_bwd_gather": (i32, [C.POINTER(RoiLevel), i32, i64, i64, p, p, p, p, i64, i32, i32, i32, p]),
    "mtp_rbox_delta_encode": (i32, [p, p, C.POINTER(f32), C.POINTER(f32), i64, p, p]),
    "mtp_rbox_delta_decode": (i32, [p, p, C.POINTER(f32), C.POINTER(f32), i64, p, p]),
    "mtp_roi_loss_workspace_bytes": (i64, [i64, i64]),
    "mtp_roi_loss": (i32, [p, i64, p, i64, i64, p, p, p, i64, p, p, p, i64, i64, C.POINTER(f32), C.POINTER(f32), f32, f32, f32, p, p, p, p, i64, p]),
    "mtp_roi_predict": (i32, [p, i64, p, i64, i64, p, i64, C.POINTER(f32), C.POINTER(f32), f32, p, p, p, p]),
    "mtp_roi_align_fwd": (i32, [C.POINTER(RoiLevel), i32, i64, i64, p, p, p, i64, i64, i32, i32, i32, f32, p, p, p]),
    "mtp_roi_align_bwd": (i32, [C.POINTER(RoiLevel), i32, i64, i64, p, p, p, p, i64, i64, i32, i32, i32, f32, i32, p]),
    "mtp_mask_loss": (i32, [p, i64, i64, i32, p, p, p, p, i64, i64, p, i64, i64, i64, p, f32, p, p, p, p, p, p]),
    "mtp_mask_paste": (i32, [p, i64, i32, p, p, i64, i64, i64, f32, i32, p, p, p]),
    "mtp_hbox_delta_encode": (i32, [p, p, C.POINTER(f32), C.POINTER(f32), i64, p, p]),
    "mtp_hbox_delta_decode": (i32, [p, p, C.POINTER(f32), C.POINTER(f32), f32, i64, p, p, i64, p, p]),
    "mtp_hrpn_loss_workspace_bytes": (i64, [i64, i64]),
    "mtp_hrpn_loss": (i32, [C.POINTER(RpnLevel), i32, i64, p, i64, p, i64, p, p, p, p, i64, i64, C.POINTER(f32), C.POINTER(f32), f32, f32, p, p, p, i64, p]),
    "mtp_hrpn_proposals": (i32, [C.POINTER(RpnLevel), i32, i64, p, i64, p, i64, C.POINTER(f32), C.POINTER(f32), f32, p, f32, p, p, p, p, p]),
    "mtp_hroi_loss_workspace_bytes": (i64, [i64, i64]),
    "mtp_hroi_loss": (i32, [p, i64, p, i64, i64, p, p, p, i64, p, p, p, i64, i64, C.POINTER(f32), C.POINTER(f32), i32, f32, f32, p, p, p, p, i64, p]),
    "mtp_hroi_predict": (i32, [p, i64, p, i64, i64, p, i64, C.POINTER(f32), C.POINTER(f32), f32, p, p, i64, f32, p, p, p, p]),
    "mtp_version": (C.c_char_p, []),
    "mtp_stream_create_low_priority": (i32, [p]),
    "mtp_stream_create_cu_mask": (i32, [p, i32, p]),
    "mtp_probe_placement": (i32, [p, i32, i64, p]),
    "mtp_stream_destroy": (i32, [p]),
}

_lib = None


class MtpHipError(RuntimeError):
    pass


def load():
    """Load libmtp_hip.so and bind every symbol; raises if the HIP extension is missing (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MtpHipError("libmtp_hip.so not found at %s -- build it first (__graft_entry__.build() or make -C mtp_amd/csrc); "
                          "mtp_amd has no CPU/PyTorch fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    ab = bool(os.environ.get("MTP_HIP_LIB"))
    for name, (res, args) in SIGNATURES.items():
        if ab and not hasattr(lib, name):
            continue              # an A/B build of an older tree (tools/_abl): entry points added since are simply absent
        fn = getattr(lib, name)   # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        kind = {-1: "invalid argument", -2: "unsupported configuration"}.get(rc, "hipError_t %d" % rc)
        raise MtpHipError("%s failed: %s" % (what, kind))
