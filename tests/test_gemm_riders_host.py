"""CPU: the host side of the NT GEMM riders -- how many workgroups run the GEMM (mtp_nt_p8_gemm_wgs), what mtp_gemm_nt_rider refuses before it launches, and
the decision it launches by (mtp_gemm_nt_rider_plan): the fallback gives the same bits as a riding launch, so a wrong turn there fails no numeric test.
Every expected value of the decision table is worked out by hand from the rule, next to the case."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from mtp_amd import _lib
    return _lib.load()


# ntiles, cus -> GEMM workgroups (the other cus - result CUs are spare): the fewest workgroups that finish in ceil(ntiles / cus) rounds
WGS = [(224, 256, 224), (672, 256, 224), (896, 256, 224), (196, 256, 196), (784, 256, 196), (256, 256, 256), (1024, 256, 256), (40, 256, 40), (672, 128, 112)]


@pytest.mark.parametrize("ntiles,cus,wgs", WGS)
def test_gemm_workgroups_of_a_launch_with_riders(lib, ntiles, cus, wgs):
    assert lib.mtp_nt_p8_gemm_wgs(ntiles, cus) == wgs
    rounds = -(-ntiles // cus)
    assert wgs <= cus and -(-ntiles // wgs) == rounds and (wgs == 1 or -(-ntiles // (wgs - 1)) > rounds)      # same rounds, and no fewer workgroups would do


def test_gemm_workgroups_rejects_nonpositive_arguments(lib):
    assert lib.mtp_nt_p8_gemm_wgs(0, 256) == -1 and lib.mtp_nt_p8_gemm_wgs(224, 0) == -1 and lib.mtp_nt_p8_gemm_wgs(-3, -1) == -1


def _fake_call(kind, act_dtype=1, **over):
    """a call whose pointers are fake (never dereferenced on the host) and whose sizes pass every check"""
    from mtp_amd import _lib
    P = 1 << 20
    g = _lib.GemmArgs(A=P, B=P, C=P, M=448, N=512, K=128, lda=128, ldb=128, ldc=512, in_dtype=_lib.MTP_BF16, out_dtype=_lib.MTP_BF16, epilogue=_lib.EPI_BIAS,
                      split_k=1)
    r = _lib.NtRider(kind=kind, act_dtype=act_dtype, x=P, dsamp=P, w=P, bias=P, avg=P, pooled=P, samp=P, g=P, B=3, Hp=14, Wp=14, windows=12, C=128, N=10)
    for k, v in over.items():
        setattr(r, k, v)
    return g, r


def test_rider_entry_point_refuses_bad_arguments_before_launching(lib):
    """NULL arguments, an unknown kind and sizes the stand-alone entry points refuse: MTP_ERR_ARG; an activation dtype other than bf16: MTP_ERR_UNSUPPORTED.
    A launch attempt without a device would come back as a positive hipError_t."""
    import torch
    from mtp_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("fake device pointers: only where a launch cannot reach a device")
    assert _lib.MTP_BF16 == 1
    g, r = _fake_call(_lib.NT_RIDER_SAMPLING_FWD)
    assert lib.mtp_gemm_nt_rider(None, None, None) == -1
    assert lib.mtp_gemm_nt_rider(C.byref(g), None, None) == -1 and lib.mtp_gemm_nt_rider(None, C.byref(r), None) == -1
    for bad in (0, 2, 7):      # f32, f64, nothing
        g, r = _fake_call(_lib.NT_RIDER_SAMPLING_FWD, act_dtype=bad)
        assert lib.mtp_gemm_nt_rider(C.byref(g), C.byref(r), None) == -2, bad
    g, r = _fake_call(9)
    assert lib.mtp_gemm_nt_rider(C.byref(g), C.byref(r), None) == -1
    for kind, field in ((_lib.NT_RIDER_SAMPLING_FWD, "x"), (_lib.NT_RIDER_SAMPLING_FWD, "samp"), (_lib.NT_RIDER_SAMPLING_FWD, "C"), (_lib.NT_RIDER_SAMPLING_FWD, "Hp"),
                        (_lib.NT_RIDER_SAMPLING_BWD_WIN, "dsamp"), (_lib.NT_RIDER_SAMPLING_BWD_WIN, "g"), (_lib.NT_RIDER_SAMPLING_BWD_WIN, "windows"),
                        (_lib.NT_RIDER_SAMPLING_BWD_WIN, "N")):
        g, r = _fake_call(kind, **{field: 0})
        assert lib.mtp_gemm_nt_rider(C.byref(g), C.byref(r), None) == -1, (kind, field)
    g, r = _fake_call(_lib.NT_RIDER_SAMPLING_FWD, C=130)       # channels in whole quads
    assert lib.mtp_gemm_nt_rider(C.byref(g), C.byref(r), None) == -1
    g, r = _fake_call(_lib.NT_RIDER_SAMPLING_BWD_WIN)
    g.A = None                                                   # the GEMM's own checks still hold under a valid rider
    assert lib.mtp_gemm_nt_rider(C.byref(g), C.byref(r), None) == -1


def test_rider_struct_mirrors_the_header():
    import os
    import re
    from conftest import ROOT
    from mtp_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtp_hip.h")).read(), flags=re.S)
    body = re.search(r"struct mtp_nt_rider \{([^}]*)\};", src).group(1)
    # "const float* w;" / "int64_t B, Hp, Wp;": the names are what is left of a declaration without its type words
    fields = [n for decl in body.split(";") for n in re.sub(r"\b(const|void|float|int|int64_t)\b|[\*,]", " ", decl).split()]
    assert fields == [f for f, _ in _lib.NtRider._fields_]
    assert C.sizeof(_lib.NtRider) == 8 + 8 * 8 + 6 * 8
    kinds = dict(re.findall(r"MTP_(NT_RIDER_[A-Z_]+) = (\d+)", src))
    assert {k: int(v) for k, v in kinds.items()} == {n: getattr(_lib, n) for n in dir(_lib) if n.startswith("NT_RIDER_")} and len(kinds) == 3


def test_rider_plan_struct_mirrors_the_header():
    import os
    import re
    from conftest import ROOT
    from mtp_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtp_hip.h")).read(), flags=re.S)
    fields = re.findall(r"int (\w+);", re.search(r"struct mtp_nt_rider_plan \{([^}]*)\};", src).group(1))
    assert fields == [f for f, _ in _lib.NtRiderPlan._fields_] == ["rides", "gemm_wgs", "riders", "windows_per_rider", "scratch_bytes", "reason"]
    assert C.sizeof(_lib.NtRiderPlan) == 4 * len(fields)
    reasons = dict(re.findall(r"MTP_(NT_RIDE_[A-Z_]+) = (\d+)", src))
    assert {k: int(v) for k, v in reasons.items()} == {n: getattr(_lib, n) for n in dir(_lib) if n.startswith("NT_RIDE_")} and len(reasons) == 5
    assert (_lib.NT_RIDE_OK, _lib.NT_RIDE_NO_FAMILY, _lib.NT_RIDE_NO_INSTANTIATION, _lib.NT_RIDE_NO_SPARE_CU, _lib.NT_RIDE_NO_SCRATCH) == (0, 1, 2, 3, 4)
    assert _lib.SIGNATURES["mtp_gemm_nt_rider_plan"][1][2] is C.c_int and callable(ops.gemm_nt_rider_plan)


# ---- the decision table of mtp_gemm_nt_rider_plan, `cus` given: no device is touched ------------------------------------------------------------------
P = 1 << 20      # a fake pointer: non-NULL, 16-byte aligned, never dereferenced by a query
OK, NO_FAMILY, NO_INST, NO_SPARE, NO_SCRATCH = 0, 1, 2, 3, 4
LDS = 160 * 1024      # dynamic LDS of the rider instantiations: the 128-KiB ring + 8 x 4 KiB of epilogue regions


def _gemm(M, N, K, bias=True, variant=0, in_dtype=1, out_dtype=1, epilogue=0):
    from mtp_amd import _lib
    return _lib.GemmArgs(A=P, B=P, C=P, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, in_dtype=in_dtype, out_dtype=out_dtype, epilogue=epilogue, bias=P if bias else None,
                         split_k=1, variant=variant)


def _fwd(B, Cc, N, Hp=14, Wp=14):
    """14 x 14 tokens are 2 x 2 windows of 7 x 7: 4 B windows"""
    from mtp_amd import _lib
    return _lib.NtRider(kind=_lib.NT_RIDER_SAMPLING_FWD, act_dtype=_lib.MTP_BF16, x=P, w=P, bias=P, avg=P, pooled=P, samp=P, B=B, Hp=Hp, Wp=Wp, C=Cc, N=N)


def _bwd(windows, Cc, N):
    from mtp_amd import _lib
    return _lib.NtRider(kind=_lib.NT_RIDER_SAMPLING_BWD_WIN, act_dtype=_lib.MTP_BF16, dsamp=P, w=P, avg=P, g=P, windows=windows, C=Cc, N=N)


def _none():
    from mtp_amd import _lib
    return _lib.NtRider(kind=_lib.NT_RIDER_NONE)


def _plan(lib, g, r, cus):
    from mtp_amd import _lib
    out = _lib.NtRiderPlan(rides=-7, gemm_wgs=-7, riders=-7, windows_per_rider=-7, scratch_bytes=-7, reason=-7)
    assert lib.mtp_gemm_nt_rider_plan(C.byref(g), C.byref(r), cus, C.byref(out)) == 0
    return (out.rides, out.gemm_wgs, out.riders, out.windows_per_rider, out.scratch_bytes, out.reason)


def _nt_plan(lib, g, cus):
    from mtp_amd import _lib
    out = _lib.GemmNtPlan()
    assert lib.mtp_gemm_nt_plan(C.byref(g), cus, C.byref(out)) == 0
    return (out.family, out.tile_m, out.persistent, out.store_policy)


def test_the_two_engine_launches_ride_under_the_default_dispatch_on_256_cus(lib):
    """ViT-L at B = 64: 12544 tokens, 256 windows, C = 1024, 16 heads (N = 80), variant 0 -- what engine.py launches.
    qkv forward 12544 x 3072 x 1024: 588 tiles of 256 rows cost 3 rounds x 256, 56 x 12 = 672 tiles of 224 rows 3 rounds x 224: 224-row tiles, 672 > 256:
    persistent.  ceil(672 / 3) = 224 GEMM workgroups, 32 spare, 32 riders, 256 / 32 = 8 windows each, 8 pooled rows x 4 x 1024 B.
    dqkv 12544 x 1024 x 3072, no bias: 196 tiles of 256 rows cost 256, 56 x 4 = 224 of 224 rows cost 224: 224-row tiles, 224 <= 256: one round, not persistent.
    224 workgroups, 32 riders, 8 windows each, 2 x (4096 + 80 x 4) B."""
    from mtp_amd import _lib
    fwd, dq = _gemm(12544, 3072, 1024), _gemm(12544, 1024, 3072, bias=False)
    assert _nt_plan(lib, fwd, 256) == (_lib.GEMM_NT_FAMILY_P8, 224, 1, 1) and _nt_plan(lib, dq, 256) == (_lib.GEMM_NT_FAMILY_P8, 224, 0, 1)
    assert _plan(lib, fwd, _fwd(64, 1024, 80), 256) == (1, 224, 32, 8, 8 * 4 * 1024, OK)
    assert _plan(lib, dq, _bwd(256, 1024, 80), 256) == (1, 224, 32, 8, 2 * (4096 + 320), OK)
    # the even walk alone (tools/ab_nt_riders.py): the same 224 workgroups, nobody rides.  Only a persistent launch has a walk to even out: on the one-round
    # plan MTP_NT_RIDER_NONE is the ordinary launch (one tile per workgroup either way)
    assert _plan(lib, fwd, _none(), 256) == (1, 224, 0, 0, 0, OK) and _plan(lib, dq, _none(), 256) == (0, 0, 0, 0, 0, NO_INST)


def test_the_two_engine_launches_on_a_128_cu_stream_fall_back(lib):
    """The same launches on half the chip (a CU-masked stream of 128): NEITHER rides, and it is the plan that says so, not the CU count.
    qkv forward: 588 tiles of 256 rows are 5 rounds x 256 = 1280, 672 of 224 rows 6 rounds x 224 = 1344: the dispatch takes 256-row tiles, which have no
    rider instantiation (and are not persistent).  dqkv: 196 x 256 rows = 2 rounds x 256 = 512 against 224 x 224 rows = 2 x 224 = 448: 224-row tiles, but
    224 tiles > 128 CUs makes the launch persistent, and the backward rider exists for the one-round form only.  Both run as GEMM, then stand-alone kernel."""
    from mtp_amd import _lib
    fwd, dq = _gemm(12544, 3072, 1024), _gemm(12544, 1024, 3072, bias=False)
    assert _nt_plan(lib, fwd, 128) == (_lib.GEMM_NT_FAMILY_P8, 256, 0, 3) and _nt_plan(lib, dq, 128) == (_lib.GEMM_NT_FAMILY_P8, 224, 1, 1)
    assert _plan(lib, fwd, _fwd(64, 1024, 80), 128) == (0, 0, 0, 0, 0, NO_INST)
    assert _plan(lib, dq, _bwd(256, 1024, 80), 128) == (0, 0, 0, 0, 0, NO_INST)


def _v(persist):
    from mtp_amd import _lib
    return _lib.GEMM_NT_P8_224 | (_lib.GEMM_NT_PERSIST if persist else _lib.GEMM_NT_NO_PERSIST)


# (tile rows, tile columns, cus, windows = 4 B) -> gemm_wgs, riders, windows per rider; K = 128, C = 128, N = 10 (forward scratch: rows x 512 B, rows = per
# rounded up to 4; backward: 2 x (4096 + 48) B)
SPARE = [
    (1, 127, 128, 36, 127, 1, 36),      # spare 1: one rider takes all 36 windows
    (1, 120, 128, 36, 120, 8, 5),       # spare 8: 36 / 8 -> 5, an odd count that is no multiple of 4
    (1, 88, 128, 36, 88, 32, 2),        # spare 40: capped at 32 riders
    (1, 88, 128, 12, 88, 12, 1),        # fewer windows than riders to lend: one rider per window
    (2, 129, 256, 256, 129, 32, 8),     # 258 tiles on 256 CUs: two rounds, ceil(258 / 2) = 129 workgroups walk two tiles each (persistent form only)
    (2, 257, 256, 256, 172, 32, 8),     # 514 tiles: three rounds, ceil(514 / 3) = 172
]


@pytest.mark.parametrize("tm,tn,cus,windows,wgs,riders,per", SPARE)
def test_rider_plan_spare_cus_riders_and_trip_counts(lib, tm, tn, cus, windows, wgs, riders, per):
    rows = -(-per // 4) * 4
    assert _plan(lib, _gemm(224 * tm, 256 * tn, 128, variant=_v(1)), _fwd(windows // 4, 128, 10), cus) == (1, wgs, riders, per, rows * 4 * 128, OK)
    if tm * tn <= cus:      # the backward rider: one tile per workgroup, one round
        assert _plan(lib, _gemm(224 * tm, 256 * tn, 128, bias=False, variant=_v(0)), _bwd(windows, 128, 10), cus) == (1, tm * tn, riders, per, 2 * (4096 + 48), OK)


def test_rider_plan_without_a_spare_cu(lib):
    """128 tiles on 128 CUs: every CU has a GEMM workgroup.  A one-round plan of 130 tiles on 128 CUs runs in two waves: no CU is idle from the start, and
    there is no GEMM workgroup count to report.  Without riders to place (MTP_NT_RIDER_NONE) the full launch is still the rider instantiation's."""
    assert _plan(lib, _gemm(448, 16384, 128, variant=_v(1)), _fwd(9, 128, 10), 128) == (0, 128, 0, 0, 0, NO_SPARE)
    assert _plan(lib, _gemm(448, 16384, 128, variant=_v(0)), _bwd(36, 128, 10), 128) == (0, 128, 0, 0, 0, NO_SPARE)
    assert _plan(lib, _gemm(448, 16640, 128, variant=_v(0)), _bwd(36, 128, 10), 128) == (0, 0, 0, 0, 0, NO_SPARE)
    assert _plan(lib, _gemm(448, 16384, 128, variant=_v(1)), _none(), 128) == (1, 128, 0, 0, 0, OK)
    assert _plan(lib, _gemm(448, 16640, 128, variant=_v(0)), _none(), 128) == (0, 0, 0, 0, 0, NO_INST)      # (no even walk of a one-round plan)


def test_rider_plan_names_family_and_instantiation(lib):
    from mtp_amd import _lib
    f, b = _fwd(3, 128, 10), _bwd(12, 128, 10)
    # 4 tiles under the default dispatch: the 128-wide family; K = 64 is half a K-tile pair: P8 refuses even when forced; an f32 GEMM
    assert _plan(lib, _gemm(448, 512, 128), f, 256) == (0, 0, 0, 0, 0, NO_FAMILY)
    assert _plan(lib, _gemm(448, 512, 64, variant=_v(1)), f, 256) == (0, 0, 0, 0, 0, NO_FAMILY)
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(1), in_dtype=_lib.MTP_F32, out_dtype=_lib.MTP_F32), f, 256) == (0, 0, 0, 0, 0, NO_FAMILY)
    # P8, but: persistence the wrong way round for the kind; 256-row tiles; plain stores; an f32 output; another epilogue
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(0)), f, 256) == (0, 0, 0, 0, 0, NO_INST)
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(1)), b, 256) == (0, 0, 0, 0, 0, NO_INST)
    assert _plan(lib, _gemm(512, 512, 128, variant=_lib.GEMM_NT_P8_256 | _lib.GEMM_NT_PERSIST), f, 256) == (0, 0, 0, 0, 0, NO_INST)
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(1) | _lib.GEMM_STORE_PLAIN), f, 256) == (0, 0, 0, 0, 0, NO_INST)
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(1), out_dtype=_lib.MTP_F32), f, 256) == (0, 0, 0, 0, 0, NO_INST)
    g = _gemm(448, 512, 128, variant=_v(1), epilogue=_lib.EPI_MUL)
    g.aux, g.aux_ld = P, 512
    assert _plan(lib, g, f, 256) == (0, 0, 0, 0, 0, NO_INST)
    # and the two that do ride: 4 tiles, 252 spare CUs, 12 windows
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(1)), f, 256) == (1, 4, 12, 1, 4 * 4 * 128, OK)
    assert _plan(lib, _gemm(448, 512, 128, variant=_v(0)), b, 256) == (1, 4, 12, 1, 2 * (4096 + 48), OK)


def test_rider_plan_scratch_limit(lib):
    """forward: rows x 4 C bytes with rows in whole groups of 4, against the launch's 160 KiB.  The widest head (C = 8192, the entry point's limit) fits with
    up to 4 windows per rider (128 KiB) and with 5 to 8 does not (256 KiB); 8 rows fit up to C = 5120 (exactly 160 KiB).  120 tiles on 128 CUs: 8 riders."""
    g = _gemm(224, 256 * 120, 128, variant=_v(1))
    assert _plan(lib, g, _fwd(3, 8192, 10), 128) == (1, 120, 8, 2, 4 * 4 * 8192, OK)
    assert _plan(lib, g, _fwd(8, 8192, 10), 128) == (1, 120, 8, 4, 128 * 1024, OK)
    for B, per in ((9, 5), (10, 5), (11, 6), (13, 7), (16, 8)):
        assert _plan(lib, g, _fwd(B, 8192, 10), 128) == (0, 120, 8, per, 256 * 1024, NO_SCRATCH), B
    assert _plan(lib, g, _fwd(16, 5120, 10), 128) == (1, 120, 8, 8, LDS, OK)
    assert _plan(lib, g, _fwd(16, 5124, 10), 128) == (0, 120, 8, 8, 8 * 4 * 5124, NO_SCRATCH)
    # backward: 2 x (4096 + 4 N rounded up to 16), N <= 4096 by the entry point's own check: always fits
    gb = _gemm(224, 256 * 120, 128, bias=False, variant=_v(0))
    assert _plan(lib, gb, _bwd(36, 128, 4096), 128) == (1, 120, 8, 5, 2 * (4096 + 16384), OK)
    assert _plan(lib, gb, _bwd(36, 128, 5), 128) == (1, 120, 8, 5, 2 * (4096 + 32), OK)


def test_rider_plan_refuses_what_the_launch_refuses(lib):
    from mtp_amd import _lib
    g, f, out = _gemm(448, 512, 128, variant=_v(1)), _fwd(3, 128, 10), _lib.NtRiderPlan()
    q = lib.mtp_gemm_nt_rider_plan
    assert q(None, C.byref(f), 256, C.byref(out)) == -1 and q(C.byref(g), None, 256, C.byref(out)) == -1 and q(C.byref(g), C.byref(f), 256, None) == -1
    bad = _fwd(3, 128, 10)
    bad.act_dtype = _lib.MTP_F32
    assert q(C.byref(g), C.byref(bad), 256, C.byref(out)) == -2
    for r in (_fwd(3, 130, 10), _fwd(3, 8196, 10), _fwd(0, 128, 10), _bwd(12, 128, 4097), _bwd(0, 128, 10), _lib.NtRider(kind=9)):
        assert q(C.byref(g), C.byref(r), 256, C.byref(out)) == -1
    g.A = None
    assert q(C.byref(g), C.byref(f), 256, C.byref(out)) == -1
    g = _gemm(448, 512, 128, variant=_v(1))
    g.bias_mod = 6
    assert q(C.byref(g), C.byref(f), 256, C.byref(out)) == -1


# ---- the element-wise bounds of tests/test_hip_gemm_riders.py, confirmed the way such a bound has to be: a float32 evaluation of the float64 reference, on the
# very inputs of the GPU tests, stays inside them with room to spare, so an f32 kernel that evaluates the same formulas in another order can meet them
def _gpu_cases():
    import test_hip_gemm_riders as R
    fwd = sorted(set(R.SAMPLERS + [s for s, _ in R.TRIPS] + [(3, 14, 14, 1024, 16), (3, 14, 14, 768, 12), (3, 14, 14, 1280, 3), (8, 14, 14, 8192, 2), (9, 14, 14, 8192, 2)]))
    bwd = [(12, 1024, 80), (12, 1280, 15), (12, 128, 5), (12, 128, 4096), (36, 128, 10), (256, 128, 10), (160, 128, 10), (96, 128, 10), (36, 256, 20)]
    return fwd, bwd


@pytest.mark.parametrize("sampler", _gpu_cases()[0])
def test_forward_rider_bounds_hold_for_a_float32_evaluation(sampler):
    import torch
    import test_hip_gemm_riders as R
    B, Hp, Wp, Cc, heads = sampler
    case = R.fwd_case(*sampler)
    avg, pooled, samp, _ = R.fwd_eval(case["x"], case["ws"], case["bs"], B, Hp, Wp, torch.float32)
    for name, got in (("avg", avg), ("pooled", pooled), ("samp", samp)):
        err, bound = (got.double() - case[name]).abs(), case[name + "_b"]
        assert bool((bound > 0).all()) and bool((err <= 0.5 * bound).all()), (name, float((err / bound).max()))      # half: a kernel's other order of summation has room


@pytest.mark.parametrize("R_,Cc,N", _gpu_cases()[1])
def test_backward_rider_bound_holds_for_a_float32_evaluation(R_, Cc, N):
    import torch
    import test_hip_gemm_riders as R
    case = R.bwd_case(R_, Cc, N)
    err = (R.bwd_eval(case["dsamp"], case["ws"], case["avg"], torch.float32).double() - case["g"]).abs()
    assert bool((case["g_b"] > 0).all()) and bool((err <= 0.5 * case["g_b"]).all()), float((err / case["g_b"]).max())
