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
