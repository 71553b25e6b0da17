"""CPU: the host side of the NT GEMM riders -- how many workgroups run the GEMM (mtp_nt_p8_gemm_wgs) and what mtp_gemm_nt_rider refuses before it launches."""
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
