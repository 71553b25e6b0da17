"""CPU: the C-ABI library loads and exports every symbol include/mtp_hip.h declares (no compute calls)."""
import os
import re

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "mtp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mtp_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_bound_and_exported():
    from mtp_amd import _lib
    names = _declared()
    assert len(names) >= 25
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and include/mtp_hip.h disagree"
    lib = _lib.load()                     # raises if libmtp_hip.so is missing: there is no fallback
    for n in names:
        assert getattr(lib, n) is not None
    assert b"gfx950" in lib.mtp_version()


def test_gemm_variant_flags_mirror_the_header():
    """enum mtp_gemm_variant / mtp_gemm_nt_family and struct mtp_gemm_nt_plan against their mirrors in _lib (and the re-exports of ops' namespace)"""
    import ctypes as C
    from mtp_amd import _lib
    src = open(os.path.join(ROOT, "include", "mtp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for enum, floor in (("mtp_gemm_variant", 25), ("mtp_gemm_nt_family", 5)):
        body = re.search(r"typedef enum \{([^}]*)\}\s*%s;" % enum, src).group(1)
        items = re.findall(r"MTP_(GEMM_[A-Z0-9_]+)\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*(?:,|$)", body)
        assert len(items) >= floor and len(items) == body.count("="), enum
        for name, v, sh in items:
            assert getattr(_lib, name) == int(v) << int(sh or 0), name
        mirrored = [n for n in dir(_lib) if n.startswith("GEMM_") and (n.startswith("GEMM_NT_FAMILY_") == (enum == "mtp_gemm_nt_family"))]
        assert sorted(mirrored) == sorted(n for n, _, _ in items), enum
    # today's numbers are ABI: A/B libraries and recorded profiles refer to them
    assert (_lib.GEMM_NT_REG_STAGED, _lib.GEMM_NT_SB8 | _lib.GEMM_ORDER_GROUPED, _lib.GEMM_NT_P8_224 | _lib.GEMM_ORDER_PLAIN, _lib.GEMM_NT_NO_P8) == (1, 36, 514, 1024)
    assert (_lib.GEMM_NT_PERSIST, _lib.GEMM_NT_STRIP, _lib.GEMM_TNG_PLAIN_PHASES, _lib.GEMM_STORE_PLAIN, _lib.GEMM_TN_REG_TRANSPOSE) == (32768, 1 << 17, 1 << 19, 3 << 20, 16)
    fields = re.findall(r"int (\w+);", re.search(r"struct mtp_gemm_nt_plan \{([^}]*)\};", src).group(1))
    assert fields == [f for f, _ in _lib.GemmNtPlan._fields_] and C.sizeof(_lib.GemmNtPlan) == 4 * len(fields)


def test_conv_and_dcnv3_kernel_queries_mirror_the_header():
    """enum mtp_conv_op / mtp_conv_kernel_family / mtp_dcnv3_kernel_family against their mirrors in _lib and the name tables of ops / ops_dcnv3; the two
    queries are stream-less host functions that refuse NULL pointers, a NULL geometry and an unknown operator like the entry points they speak for"""
    import ctypes as C
    from mtp_amd import _lib, ops
    from mtp_amd.ops_dcnv3 import DCNV3_KERNEL
    src = open(os.path.join(ROOT, "include", "mtp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for enum, prefix, count in (("mtp_conv_op", "CONV_OP_", 5), ("mtp_conv_kernel_family", "CONV_KERNEL_", 5), ("mtp_dcnv3_kernel_family", "DCNV3_", 11)):
        body = re.search(r"typedef enum \{([^}]*)\}\s*%s;" % enum, src).group(1)
        items = re.findall(r"MTP_([A-Z0-9_]+)\s*=\s*(\d+)\s*(?:,|$)", body)
        assert len(items) == count == body.count("="), enum
        for name, v in items:
            assert name.startswith(prefix) and getattr(_lib, name) == int(v), name
        assert sorted(n for n in dir(_lib) if n.startswith(prefix)) == sorted(n for n, _ in items), enum
    assert ops.CONV_KERNEL == {n[len("CONV_KERNEL_"):].lower(): getattr(_lib, n) for n in dir(_lib) if n.startswith("CONV_KERNEL_") and n != "CONV_KERNEL_NONE"}
    assert DCNV3_KERNEL == {n[len("DCNV3_"):].lower(): getattr(_lib, n) for n in dir(_lib) if n.startswith("DCNV3_") and n != "DCNV3_KERNEL_NONE"}
    assert sorted(ops._CONV_OP.values()) == [0, 1, 2, 3, 4]
    for name in ("mtp_conv_kernel", "mtp_dcnv3_kernel"):
        assert C.c_void_p not in _lib.SIGNATURES[name][1][-1:], name        # no trailing stream argument
    lib = _lib.load()
    g = _lib.Dcnv3Geom(N=1, H=4, W=4, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dilation_h=1, dilation_w=1, group=1, group_channels=16,
                       offset_scale=1.0, im2col_step=1)
    assert lib.mtp_dcnv3_kernel(16, 16, 16, 16, None, None, None, 0, C.byref(g), 0) == _lib.DCNV3_FWD9
    assert lib.mtp_dcnv3_kernel(16, 16, 16, 16, None, None, None, 0, C.byref(g), 1) == -1          # backward without the gradient buffers
    assert lib.mtp_dcnv3_kernel(16, 16, 16, 16, None, None, None, 0, None, 0) == -1 and lib.mtp_dcnv3_kernel(16, 16, 16, 16, None, None, None, 7, C.byref(g), 0) == -1
    assert lib.mtp_dcnv3_kernel(16, 16, 16, 16, 16, 16, 16, 2, C.byref(g), 1) == _lib.DCNV3_F64
    assert lib.mtp_conv_kernel(9, 16, 0, 0, 0, 0, 0, 16, 0, 16, None, 1, 1, 1, 4, 1, 0) == -1       # unknown operator
    assert lib.mtp_conv_kernel(_lib.CONV_OP_DWCONV3X3_FWD, 16, 1, 0, 0, 0, 0, 16, 1, 16, None, 1, 1, 8, 4, 1, 0) == _lib.CONV_KERNEL_P8
    assert lib.mtp_conv_kernel(_lib.CONV_OP_DWCONV3X3_FWD, 16, 2, 0, 0, 0, 0, 16, 2, 16, None, 1, 1, 8, 4, 1, 0) == _lib.CONV_KERNEL_NONE      # f64: unsupported


def test_attention_family_tables_mirror_the_header():
    """the anonymous enum of attention kernel families (mtp_full_attn_kernel / mtp_rvsa_attn_kernel) against the name tables of ops: names and values"""
    from mtp_amd import ops
    src = open(os.path.join(ROOT, "include", "mtp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"enum \{([^}]*MTP_ATTN_KERNEL_NONE[^}]*)\};", src).group(1)
    items = re.findall(r"MTP_([A-Z0-9_]+)\s*=\s*(\d+)\s*(?:,|$)", body)
    assert len(items) == 14 == body.count("=") and items[0] == ("ATTN_KERNEL_NONE", "0")
    for table in ("FULL_FWD", "FULL_BWD", "RVSA_FWD", "RVSA_BWD"):
        assert getattr(ops, table) == {n[len(table) + 1:].lower(): int(v) for n, v in items if n.startswith(table + "_")}, table
    assert sorted(n for n, _ in items[1:]) == sorted("%s_%s" % (t, k.upper()) for t in ("FULL_FWD", "FULL_BWD", "RVSA_FWD", "RVSA_BWD") for k in getattr(ops, t))


def test_gemm_args_struct_layout():
    import ctypes as C
    from mtp_amd._lib import GemmArgs
    # mirrors `mtp_gemm_args` in the header: 3 ptrs, 6 i64, 3 i32 (+pad), ptr, i64, ptr, 2 i64, ptr, i64, ptr, i64, 2 i32, ptr, 2 i32, ptr, i64
    assert C.sizeof(GemmArgs) == 3 * 8 + 6 * 8 + 3 * 4 + 4 + 8 + 8 + 8 + 16 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8
    assert GemmArgs.workspace.offset == 184 and GemmArgs.workspace_bytes.offset == 192
    assert GemmArgs.bias.offset == 88 and GemmArgs.split_k.offset == 160 and GemmArgs.colsum.offset == 168 and GemmArgs.defer_sum.offset == 176


def test_weight_image_descriptor_layout():
    import ctypes as C
    from mtp_amd._lib import WimgDesc
    # mtp_wimg_desc: 3 ptrs, 3 i64, 2 i32
    assert C.sizeof(WimgDesc) == 56 and WimgDesc.R.offset == 24 and WimgDesc.tile0.offset == 40 and WimgDesc.f32_out.offset == 48


def test_arg_checks_reject_without_gpu():
    """argument validation happens before any launch, so it is testable on CPU"""
    import ctypes as C
    from mtp_amd import _lib
    lib = _lib.load()
    g = _lib.GemmArgs()
    assert lib.mtp_gemm_nt(C.byref(g), None) == -1
    assert lib.mtp_gemm_tn(C.byref(g), None) == -1
    assert lib.mtp_layernorm_fwd(None, 0, None, None, None, 0, None, None, 4, 8, 1e-6, 0, None) == -1
    assert lib.mtp_full_attn_fwd(None, None, None, 0, None, None, 1, 14, 14, 2, 64, 0.125, None) == -1
    assert lib.mtp_layernorm_bwd_partial_rows(12544) == 512 and lib.mtp_layernorm_bwd_partial_rows(10) == 3


def test_every_entry_point_rejects_null_arguments_before_launching():
    """the whole ABI: all-NULL pointers / zero sizes must come back as MTP_ERR_ARG (-1) from the argument checks -- no launch,
    no dereference, no GPU needed.  (Pure query functions are exercised in the other tests.)"""
    import ctypes as C
    from mtp_amd import _lib
    lib = _lib.load()
    queries = {"mtp_version", "mtp_layernorm_bwd_partial_rows", "mtp_full_attn_bwd_workspace_floats", "mtp_dwconv3x3_bwd_dw_partial_rows",
               "mtp_scale_residual_bwd_partial_rows", "mtp_gemm_nt_workspace_bytes"}
    for name, (_, argtypes) in sorted(_lib.SIGNATURES.items()):
        if name in queries:
            continue
        args = [0.0 if a is C.c_float else (None if (a is C.c_void_p or hasattr(a, "contents")) else 0) for a in argtypes]
        assert getattr(lib, name)(*args) == -1, name


# ---- every entry point that takes a dtype refuses an unknown one before it launches --------------------------------------------------------------
# One passing argument tuple per entry point: plausible sizes, P = a non-NULL (16-byte aligned, never dereferenced) pointer, D = the dtype under test.
# With a valid dtype every tuple passes its entry point's argument checks and reaches the launch; the test puts an unknown value into every D.
_P, _D = 1 << 20, "dtype"
_DTYPE_REFUSALS = {
    "mtp_layernorm_fwd": (_P, _D, _P, _P, _P, _D, _P, _P, 4, 8, 1e-6, 0, None),
    "mtp_layernorm_bwd": (_P, _D, _P, _D, _P, _P, _P, _P, 0, None, None, _P, _D, None, _D, None, 0, _P, _P, 0, 4, 8, None),
    "mtp_layernorm_bwd_win": (_P, _D, _P, _D, _P, _P, _P, None, None, _P, _D, None, _D, None, 0, _P, _P, 0, 49, 8, _P, 1, 7, 7, None),
    "mtp_layernorm_residual_fwd": (_P, _D, _P, _P, _P, _P, None, 0, _P, _P, _P, _P, 4, 8, 1e-6, None),
    "mtp_layernorm_residual_bwd": (_P, _P, _D, _P, _P, _P, _P, _P, None, 0, _P, _P, 4, 8, None),
    "mtp_colsum": (_P, _D, 8, _P, 4, 8, None),
    "mtp_colsum_acc": (_P, _D, 8, _P, 4, 8, None),
    "mtp_patchify": (_P, _P, _D, 1, 3, 16, 16, 4, None),
    "mtp_unpatchify": (_P, _D, _P, 1, 3, 16, 16, 4, None),
    "mtp_preprocess_patchify": (_P, _P, _D, 1, 16, 16, 4, 4, "mean", "std", 0, 0.0, None),      # mean / std are read on the host: real arrays
    "mtp_cast": (_P, _D, _P, _D, 8, None),
    "mtp_transpose_cast": (_P, _P, _D, 4, 8, None),
    "mtp_weight_images": (_P, 1, 1, _D, None),
    "mtp_adamw_weight_images": (_P, 1, 1, _D, _P, _P, _P, _P, _P, None, 0.0, 1.0, None),
    "mtp_adamw_weight_images_lr": (_P, _P, 1, 1, _D, _P, _P, _P, _P, _P, None, 0.0, 1.0, None),
    "mtp_convt_pack": (_P, _P, _P, _D, 8, 8, None),
    "mtp_tokens_to_nchw": (_P, _D, _P, _D, 1, 2, 2, 8, 0, None),
    "mtp_nchw_to_tokens": (_P, _D, _P, _D, 1, 2, 2, 8, 0, None),
    "mtp_maxpool2_tokens_fwd": (_P, _P, _D, 1, 2, 2, 8, None),
    "mtp_maxpool2_tokens_bwd": (_P, _P, _D, _P, 0, 1, 2, 2, 8, None),
    "mtp_scale_rows_cast": (_P, _P, _D, None, 0, 4, 8, None),
    "mtp_im2col3x3": (_P, _D, 128, 32, 8, 1, _P, _D, 1, 4, 4, 8, 1, 72, None),
    "mtp_col2im3x3": (_P, _D, _P, 128, 32, 8, 1, 1, 4, 4, 8, 1, 72, 0, None),
    "mtp_conv3x3_pack": (_P, _P, _P, _D, 8, 8, 72, None),
    "mtp_pack_rows_padded": (_P, _P, _P, _D, 4, 8, 8, None),
    "mtp_cast_pad_rows": (_P, 4, _P, _D, 8, 4, None),
    "mtp_copy_rows": (_P, 8, _P, 8, _D, 4, 4, None),
    "mtp_dwconv3x3_fwd": (_P, _P, _P, _P, _D, 1, 4, 4, 8, None),
    "mtp_dwconv3x3_bwd_dx": (_P, _D, _P, _P, 0, 1, 4, 4, 8, None),
    "mtp_dwconv3x3_bwd_dw": (_P, _P, _D, _P, 1, 4, 4, 8, None),
    "mtp_dwconv_fwd": (_P, _P, _P, _P, _D, 1, 4, 4, 8, 5, None),
    "mtp_dwconv_bwd_dx": (_P, _D, _P, _P, 0, 1, 4, 4, 8, 5, None),
    "mtp_dwconv_bwd_dw": (_P, _P, _D, _P, _P, 1, 4, 4, 8, 5, None),
    "mtp_center_feature_scale_fwd": (_P, _P, _P, 2, _P, _D, 4, 2, 4, None),
    "mtp_center_feature_scale_bwd": (_P, _P, _P, _P, 2, _P, _P, _P, _D, 4, 2, 4, None),
    "mtp_softmax_groups_fwd": (_P, 18, _P, _D, 4, 2, 9, None),
    "mtp_softmax_groups_bwd": (_P, _P, _P, 18, _D, 4, 2, 9, None),
    "mtp_scale_residual_fwd": (_P, _P, _D, _P, None, 0, _P, _P, 4, 8, None),
    "mtp_scale_residual_bwd": (_P, _P, _D, _P, None, 0, _P, _P, 4, 8, None),
    "mtp_full_attn_fwd": (_P, _P, _P, _D, _P, _P, 1, 14, 14, 2, 64, 0.125, None),
    "mtp_full_attn_bwd": (_P, _P, _P, _P, _P, _D, _P, _P, _P, _P, 1, 14, 14, 2, 64, 0.125, None),
    "mtp_full_attn_kernel": (_D, 14, 14, 0),
    "mtp_rvsa_attn_kernel": (_D, 14, 14, 2, 0),
    "mtp_rvsa_pool_fwd": (_P, _D, _P, _P, 1, 7, 7, 8, None),
    "mtp_rvsa_pool_bwd": (_P, _P, _P, _D, 0, 1, 7, 7, 8, None),
    "mtp_rvsa_sampling_fwd": (_P, _D, _P, _P, _P, _P, _P, 1, 7, 7, 8, 4, None),
    "mtp_rvsa_sampling_bwd": (_P, _P, _P, _P, _D, 1, 7, 7, 8, 4, None),
    "mtp_rvsa_attn_fwd": (_P, _P, _P, _P, _D, _P, _P, _P, 1, 7, 7, 2, 64, 0.125, None),
    "mtp_rvsa_attn_bwd": (_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _P, _P, _P, 1, 7, 7, 2, 64, 0.125, None),
    "mtp_dcnv3_fwd": (_P, _P, _P, _P, _D, "geom", None),
    "mtp_dcnv3_bwd": (_P, _P, _P, _P, _D, _P, _P, _P, "geom", None),
    "mtp_dcnv3_bwd_act": (_P, _P, _P, _P, _D, _P, _P, _P, _P, 18, "geom", None),
    "mtp_dcnv3_kernel": (_P, _P, _P, _P, None, None, None, _D, "geom", 0),
    "mtp_comm_allreduce_bucket_dt": (_P, _P, 8, _D, None),
    "mtp_comm_reduce_scatter_bucket": (_P, _P, 8, 0, _D, None),
    "mtp_comm_allgather_bucket": (_P, _P, 8, 0, _D, None),
    "mtp_bn_stats": (_P, _D, 8, None, _P, _P, 4, 8, None),
    "mtp_bn_apply": (_P, _D, 8, _P, _P, _P, _P, 0, _P, _D, 8, 4, 8, None),
    "mtp_bn_bwd_stats": (_P, _D, 8, _P, _D, 8, _P, _P, _P, _P, 0, _P, _P, 4, 8, None),
    "mtp_bn_bwd_dx": (_P, _D, 8, _P, _D, 8, _P, _P, _P, _P, 0, None, 0.0, _P, _D, 8, 4, 8, None),
    "mtp_resize_bilinear_fwd": (_P, _D, 8, _P, _D, 8, 1, 2, 2, 4, 4, 8, 0, None),
    "mtp_resize_bilinear_bwd": (_P, _D, 8, _P, 8, 1, 2, 2, 4, 4, 8, 0, None),
    "mtp_adaptive_avg_pool_fwd": (_P, _D, 8, _P, _D, 1, 4, 4, 8, 2, None),
    "mtp_adaptive_avg_pool_bwd": (_P, _D, _P, 8, 1, 4, 4, 8, 2, 0, None),
    "mtp_channel_scale": (_P, _D, 8, _P, 4, _P, _D, 8, 4, 8, None),
    "mtp_seg_ce": (_P, _D, 4, 1, 2, 2, 3, _P, 1, 4, 4, 255, 1.0, _P, _P, 4, _P, 1 << 16, None),
    "mtp_seg_window_accumulate": (_P, _D, 4, 1, 2, 2, 3, _P, 4, 4, 4, 0, 0, 4, 4, None),
    "mtp_fuse_pair_fwd": (_P, _D, _P, _D, 8, 1, 8, 2, 2, 1, None),
    "mtp_fuse_pair_bwd": (_P, 8, _P, _D, _P, 1, 8, 2, 2, 3, None),      # policy abs_diff: the only one that reads f
    "mtp_unet_up_cat_fwd": (_P, 8, 8, None, 0, 0, _D, _P, _D, 8, 1, 2, 2, 0, 0, None),
    "mtp_gap_fwd": (_P, _D, _P, 1, 8, 4, None),
    "mtp_gap_bwd": (_P, _P, _D, 1, 8, 4, None),
}
# not in the table: the dtype arrives inside a struct, and no other argument of a passing call can carry an unknown one
_DTYPE_IN_STRUCT = {
    "mtp_gemm_nt": "mtp_gemm_args.in_dtype / out_dtype", "mtp_gemm_tn": "mtp_gemm_args", "mtp_gemm_tn_grouped": "mtp_gemm_args",
    "mtp_gemm_nt_plan": "mtp_gemm_args", "mtp_gemm_nt_workspace_bytes": "mtp_gemm_args",
    "mtp_gemm_nt_rider": "mtp_gemm_args, mtp_nt_rider.act_dtype", "mtp_gemm_nt_rider_plan": "mtp_gemm_args, mtp_nt_rider.act_dtype",
}
# a query with its own contract (the test above pins it): an unsupported dtype is the family NONE, and a query launches nothing
_DTYPE_QUERY_NONE = "mtp_conv_kernel"


def _takes_dtype():
    """the entry points of include/mtp_hip.h with a dtype among their parameters"""
    src = open(os.path.join(ROOT, "include", "mtp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = []
    for name, params in re.findall(r"\b(mtp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        if re.search(r"\bint (\w+_)?dtype\b", params):
            out.append(name)
    return sorted(out)


def test_every_entry_point_refuses_an_unknown_dtype_before_launching():
    """dtype = 7 (nothing) and MTP_F64 (a real value that only DCNv3 takes) with every other argument valid: a negative return, i.e. the argument
    checks or the dispatcher refused.  Without a device an attempted launch comes back as a positive hipError_t, which is what this test catches;
    the pointers are fake, so with a device in sight it must not run."""
    import ctypes as C
    import pytest
    import torch
    from mtp_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("fake device pointers: only where a launch cannot reach a device")
    lib = _lib.load()
    names = _takes_dtype()
    assert len(names) >= 70
    assert sorted(set(names) - {_DTYPE_QUERY_NONE}) == sorted(_DTYPE_REFUSALS), "an entry point with a dtype and no argument tuple (or the reverse)"
    assert all(n in _lib.SIGNATURES and not re.search(r"dtype", n) for n in _DTYPE_IN_STRUCT)
    geom = _lib.Dcnv3Geom(N=1, H=4, W=4, kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, dilation_h=1, dilation_w=1, group=1,
                          group_channels=16, offset_scale=1.0, im2col_step=1)
    norm = (C.c_float * 3)(1.0, 1.0, 1.0)
    held = {"geom": C.byref(geom), "mean": norm, "std": norm}
    f64_ok = {"mtp_dcnv3_fwd", "mtp_dcnv3_bwd", "mtp_dcnv3_kernel"}
    for bad in (7, 2):
        for name, tup in sorted(_DTYPE_REFUSALS.items()):
            if bad == 2 and name in f64_ok:
                continue
            assert len(tup) == len(_lib.SIGNATURES[name][1]), name
            args = [bad if a is _D else held.get(a, a) if isinstance(a, str) else a for a in tup]
            assert getattr(lib, name)(*args) < 0, (name, bad)
        for op in range(5):
            assert lib.mtp_conv_kernel(op, _P, bad, 128, 32, 8, 1, _P, bad, _P, None, 1, 4, 4, 8, 1, 72) == _lib.CONV_KERNEL_NONE, (op, bad)
