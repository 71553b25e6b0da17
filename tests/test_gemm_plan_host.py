"""CPU: which kernel mtp_gemm_nt dispatches a problem to.  All NT families give bit-identical results, so a dispatch mistake never shows in a parity
test -- it is a silent slowdown.  tests/golden/gemm_nt_plan.json holds what the launch sites decided for every problem of a sweep BEFORE the decisions
were gathered into nt_plan (csrc/gemm.hip): recorded once from that tree by an observer at its launch sites (family, rows per tile, order, persistent,
store policy: the template arguments of the kernel that would have been launched) together with mtp_gemm_nt_tile's answer.  The plan query must
reproduce the table row for row.  Neither query needs a device (256 CUs are assumed without one) or dereferences a pointer."""
import ctypes as C
import json
import os

from conftest import ROOT

FIELDS = ("family", "tile_m", "order", "persistent", "store_policy")
EPI_BIAS_GELU, EPI_BIAS_RES, EPI_DGELU, EPI_BIAS_GELU_DG, EPI_MUL = 1, 2, 3, 4, 5


def _args(_lib, M, N, K, combo, variant):
    g = _lib.GemmArgs()
    g.A, g.B, g.C = 0x10000, 0x20000, 0x30000          # never dereferenced
    g.M, g.N, g.K, g.lda, g.ldb, g.ldc = M, N, K, K, K, N
    g.in_dtype, g.out_dtype, g.epilogue = combo["in_dtype"], combo["out_dtype"], combo["epilogue"]
    g.bias = 0x40000 if combo["bias"] else None
    if combo["epilogue"] == EPI_BIAS_RES:
        g.res, g.res_ld, g.res_mod = 0x50000, N, combo["res_mod"]
    if combo["epilogue"] in (EPI_BIAS_GELU, EPI_DGELU, EPI_BIAS_GELU_DG, EPI_MUL):
        g.aux, g.aux_ld = 0x60000, N
    g.split_k, g.variant = 1, variant
    return g


def test_nt_plan_and_tile_equal_the_recorded_dispatch():
    from mtp_amd import _lib
    lib = _lib.load()
    T = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_nt_plan.json")))
    code = {c: i for i, c in enumerate(T["alphabet"])}
    per_shape = len(T["combos"]) * len(T["variants"]) * len(T["cus"])
    assert len(T["rows"]) == len(T["shapes"]) and per_shape > 1000
    plan, seen, bad = _lib.GemmNtPlan(), set(), []
    for (M, N, K), row in zip(T["shapes"], T["rows"]):
        assert len(row) == per_shape
        it = iter(row)
        for combo in T["combos"]:
            for variant in T["variants"]:
                g = _args(_lib, M, N, K, combo, variant)
                tile = lib.mtp_gemm_nt_tile(C.byref(g))
                for cus in T["cus"]:
                    want = T["outcomes"][code[next(it)]]
                    rc = lib.mtp_gemm_nt_plan(C.byref(g), cus, C.byref(plan))
                    # a problem the launch refused has no decisions in the table: the queries must refuse it as well
                    got = dict(rc=rc, tile=tile, **{f: getattr(plan, f) if rc == 0 else -9 for f in FIELDS})
                    if got != want:
                        bad.append(((M, N, K), combo, variant, cus, got, want))
                    seen.add((want["family"], want["tile_m"], want["persistent"], want["store_policy"]))
    assert not bad, "%d rows differ, first: %r" % (len(bad), bad[:3])
    # the sweep reaches every family, both tile heights and both forms of the pipelined kernel, every store policy
    assert {s[0] for s in seen} >= {0, 1, 2, 3, 4} and {(3, 224, 0), (3, 224, 1), (3, 256, 0), (3, 256, 1)} <= {s[:3] for s in seen}
    assert {s[3] for s in seen if s[0] == 3} == {1, 2, 3}


def test_tile_is_the_plan_on_the_device_cus():
    """mtp_gemm_nt_tile = the plan's family on the device's CUs (cus <= 0), named by its tile"""
    from mtp_amd import _lib
    lib = _lib.load()
    plan = _lib.GemmNtPlan()
    bf16 = dict(in_dtype=_lib.MTP_BF16, out_dtype=_lib.MTP_BF16, epilogue=_lib.EPI_BIAS, bias=1, res_mod=0)
    for (M, N, K), variant, family, tile in (((12544, 1024, 1024), 0, _lib.GEMM_NT_FAMILY_P8, 256), ((6272, 768, 768), 0, _lib.GEMM_NT_FAMILY_STRIP, 64),
                                             ((12544, 1024, 1024), _lib.GEMM_NT_NO_P8, _lib.GEMM_NT_FAMILY_SB8, 128), ((1000, 1000, 96), 0, _lib.GEMM_NT_FAMILY_REG, 128),
                                             ((1000, 1000, 128), 0, _lib.GEMM_NT_FAMILY_SB, 128)):
        g = _args(_lib, M, N, K, bf16, variant)
        for cus in (0, -1, 256):
            assert lib.mtp_gemm_nt_plan(C.byref(g), cus, C.byref(plan)) == 0 and plan.family == family, (M, N, K, variant, cus)
        assert lib.mtp_gemm_nt_tile(C.byref(g)) == tile
    assert lib.mtp_gemm_nt_plan(C.byref(g), 0, None) == -1 and lib.mtp_gemm_nt_plan(None, 0, C.byref(plan)) == -1
