"""GPU: the NT GEMM with rider workgroups (mtp_gemm_nt_rider) against the launches it replaces, bit for bit: the GEMM output against ops.gemm_nt without a
rider, avg / pooled / samp and g against the stand-alone sampling entry points.  Every buffer is poisoned and sits between guards (guard.Arena)."""
import pytest
import torch

import guard
from mtp_amd._lib import GEMM_NT_FAMILY_P8, GEMM_NT_NO_PERSIST, GEMM_NT_P8_224, GEMM_NT_PERSIST

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
ARENA = None


@pytest.fixture(scope="module")
def ops():
    from mtp_amd import ops as o
    o.lib()
    return o


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    global ARENA
    from mtp_amd import ops as o
    ARENA = a = guard.Arena("cuda")
    monkeypatch.setattr(o, "_scratch", a.scratch)
    yield a
    ARENA = None
    torch.cuda.synchronize()
    a.check()
    a.close()


def dev(t, dtype=None):
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def e(*shape, dtype=F32):
    return ARENA.empty(*shape, dtype=dtype)


# the forward rider needs the persistent instantiation, the backward one the one-round instantiation: forced here, the shapes are far below the sizes at
# which the dispatch picks this family by itself.  448 x 512 = 4 tiles of 224 x 256 (one round), 448 x 768 = 6.
GEMMS = [(448, 512, 128), (448, 768, 256)]
# (B, Hp, Wp, C, heads): 12 windows (fewer than 32 riders: the second half of every rider workgroup is idle), 36 (the stride loop: four riders take a second
# window, the other second halves are the predicated tail), a 15 x 10 grid (padded to 21 x 14: windows that hang over the edge), the wider head
SAMPLERS = [(3, 14, 14, 128, 2), (9, 14, 14, 128, 2), (3, 15, 10, 128, 2), (9, 14, 14, 256, 4)]


def _gemm_inputs(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return dev(torch.randn(M, K, generator=g), BF16), dev(torch.randn(N, K, generator=g) * 0.1, BF16), dev(torch.randn(N, generator=g))


def _fwd_inputs(B, Hp, Wp, C, heads, seed):
    g = torch.Generator().manual_seed(seed)
    return (dev(torch.randn(B * Hp * Wp, C, generator=g), BF16), dev(torch.randn(5 * heads, C, generator=g) * 0.05), dev(torch.randn(5 * heads, generator=g)))


def _fwd_outputs(ops, B, Hp, Wp, C, heads):
    nh, nw = ops.rvsa_windows(Hp, Wp)
    R = B * nh * nw
    return e(R, C), e(R, C), e(R, 5 * heads)


def _check_fwd(ops, gemm, sampler, variant, stream=None):
    M, N, K = gemm
    B, Hp, Wp, C, heads = sampler
    a, w, bias = _gemm_inputs(M, N, K, 1)
    x, ws, bs = _fwd_inputs(B, Hp, Wp, C, heads, 2)
    ref = ops.gemm_nt(a, w, e(M, N, dtype=BF16), bias=bias, variant=variant)
    avg0, pooled0, samp0 = _fwd_outputs(ops, B, Hp, Wp, C, heads)
    ops.rvsa_sampling_fwd(x, ws, bs, avg0, pooled0, samp0, B, Hp, Wp)
    avg, pooled, samp = _fwd_outputs(ops, B, Hp, Wp, C, heads)
    out = e(M, N, dtype=BF16)
    rider = ops.sampling_fwd_rider(x, ws, bs, avg, pooled, samp, B, Hp, Wp)
    if stream is None:
        ops.gemm_nt(a, w, out, bias=bias, variant=variant, rider=rider)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops.gemm_nt(a, w, out, bias=bias, variant=variant, rider=rider)
        stream.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(avg, avg0) and torch.equal(pooled, pooled0) and torch.equal(samp, samp0)


def _check_bwd(ops, gemm, sampler, variant, stream=None):
    M, N, K = gemm
    B, Hp, Wp, C, heads = sampler
    a, w, bias = _gemm_inputs(M, N, K, 3)
    nh, nw = ops.rvsa_windows(Hp, Wp)
    R = B * nh * nw
    g = torch.Generator().manual_seed(4)
    dsamp, ws, avg = dev(torch.randn(R, 5 * heads, generator=g)), dev(torch.randn(5 * heads, C, generator=g) * 0.05), dev(torch.randn(R, C, generator=g))
    ref = ops.gemm_nt(a, w, e(M, N, dtype=BF16), bias=bias, variant=variant)
    g0 = ops.rvsa_sampling_bwd_win(dsamp, ws, avg, e(R, C))
    g1, out = e(R, C), e(M, N, dtype=BF16)
    rider = ops.sampling_bwd_win_rider(dsamp, ws, avg, g1)
    if stream is None:
        ops.gemm_nt(a, w, out, bias=bias, variant=variant, rider=rider)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops.gemm_nt(a, w, out, bias=bias, variant=variant, rider=rider)
        stream.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(g1, g0)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampling_forward_rides_the_persistent_gemm(ops, gemm, sampler):
    M, N, K = gemm
    variant = GEMM_NT_P8_224 | GEMM_NT_PERSIST
    a, w, _ = _gemm_inputs(M, N, K, 1)
    plan = ops.gemm_nt_plan(a, w, torch.empty(M, N, device="cuda", dtype=BF16), variant=variant)
    assert (plan.family, plan.tile_m, plan.persistent, plan.store_policy) == (GEMM_NT_FAMILY_P8, 224, 1, 1)      # the instantiation that carries the rider
    assert ops.lib().mtp_nt_p8_gemm_wgs(2 * (N // 256), 256) == 2 * (N // 256)                                   # one round: spare CUs on any MI355X stream
    _check_fwd(ops, gemm, sampler, variant)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampling_backward_factor_rides_the_one_round_gemm(ops, gemm, sampler):
    M, N, K = gemm
    variant = GEMM_NT_P8_224 | GEMM_NT_NO_PERSIST
    a, w, _ = _gemm_inputs(M, N, K, 3)
    plan = ops.gemm_nt_plan(a, w, torch.empty(M, N, device="cuda", dtype=BF16), variant=variant)
    assert (plan.family, plan.tile_m, plan.persistent, plan.store_policy) == (GEMM_NT_FAMILY_P8, 224, 0, 1)
    _check_bwd(ops, gemm, sampler, variant)


def test_no_spare_cu_falls_back_to_two_launches(ops):
    """a 128-CU stream and 128 tiles: every CU of the stream has a GEMM workgroup, nothing to lend"""
    st = ops.cu_mask_stream("cuda", ops.cu_mask_words("interleaved", 0))
    assert ops.lib().mtp_nt_p8_gemm_wgs(128, 128) == 128
    _check_fwd(ops, (448, 16384, 128), SAMPLERS[1], GEMM_NT_P8_224 | GEMM_NT_PERSIST, stream=st)
    _check_bwd(ops, (448, 16384, 128), SAMPLERS[1], GEMM_NT_P8_224 | GEMM_NT_NO_PERSIST, stream=st)


def test_a_problem_the_p8_family_refuses_falls_back(ops):
    """K = 64 is half a K-tile pair: the 128-wide kernels run it, the rider's stand-alone kernel follows"""
    a, w, _ = _gemm_inputs(448, 512, 64, 1)
    assert ops.gemm_nt_plan(a, w, torch.empty(448, 512, device="cuda", dtype=BF16), variant=GEMM_NT_P8_224).family != GEMM_NT_FAMILY_P8
    _check_fwd(ops, (448, 512, 64), SAMPLERS[2], GEMM_NT_P8_224 | GEMM_NT_PERSIST)
    _check_bwd(ops, (448, 512, 64), SAMPLERS[2], GEMM_NT_P8_224 | GEMM_NT_NO_PERSIST)
    # the plan the other way round (a persistent launch under the backward rider, a one-round launch under the forward one): no instantiation, same results
    _check_fwd(ops, GEMMS[0], SAMPLERS[0], GEMM_NT_P8_224 | GEMM_NT_NO_PERSIST)
    _check_bwd(ops, GEMMS[0], SAMPLERS[0], GEMM_NT_P8_224 | GEMM_NT_PERSIST)
