"""GPU: the NT GEMM with rider workgroups (mtp_gemm_nt_rider) against the launches it replaces, bit for bit: the GEMM output against ops.gemm_nt without a
rider (the same variant, and the 128-wide family), avg / pooled / samp and g against the stand-alone sampling entry points.  Every buffer is poisoned and
sits between guards (guard.Arena).

The fallback of mtp_gemm_nt_rider gives the same bits as a riding launch, so EVERY case first asks the query the launch decides by
(ops.gemm_nt_rider_plan) and asserts that it rides -- with the trip counts the case exists for -- or that it falls back for the reason the case names.
A riding case is launched three times into freshly poisoned outputs, with identical bits.

Values: every output is also compared element by element with the same operation in float64 on the CPU, computed from the dtype-rounded inputs, under
bounds that follow from the arithmetic (u = 2^-24, the unit roundoff of f32):

  C       gemm_bound of tests/test_hip_edges.py: 2 K u (|a| |w|^T + |bias|) + 2^-8 |ref| for the bf16 output.
  avg     a 49-term f32 sum of values that are exact in f32 (bf16 inputs times a 0 / 1 mask), in any order: at most 48 u sum|x|; times the rounded constant
          1 / 49: two more roundings.  50 u sum|x| / 49 <= 2 * 49 u mean|x|:   avg_bound = 2 * 49 u (sum|x| / 49).
  pooled  LeakyReLU of avg: the slope is at most 1, 0.01f and the product add two roundings (52 u mean|x|); where the f32 sum falls on the other side of
          zero than the exact one, both are below avg's error and the two branches differ by less than twice that error:   pooled_bound = 2 avg_bound.
  samp    a C-term f32 dot product of pooled and a weight row (products rounded or fused, lane sums, then one wave reduction: at most C additions deep)
          plus the bias add: (C + 1) u (|pooled| |w|^T + |bias|), and the error pooled carries in:
          samp_bound = 2 C u (|pooled| |w|^T + |bias|) + pooled_bound |w|^T.
  g       an N-term f32 dot product of a dsamp row and a weight column, times the factor 1 / 49 or 0.01 / 49 chosen by the sign of the INPUT avg (no
          branch can flip): N u for the sum, 4 u for the factor (rounded 1 / 49, rounded 0.01, two products), N + 4 <= 2 N from N = 4 on:
          g_bound = 2 N u (|dsamp| |w|) factor.

tests/test_gemm_riders_host.py confirms on the CPU that a float32 evaluation of the references stays inside these bounds for the inputs used here.
The worst |err| / bound of every case goes to record_parity (group gemm_riders)."""
import functools

import pytest
import torch

import guard
from conftest import record_parity
from mtp_amd import _lib
from mtp_amd._lib import GEMM_NT_FAMILY_P8, GEMM_NT_NO_P8, GEMM_NT_NO_PERSIST, GEMM_NT_P8_224, GEMM_NT_PERSIST, GEMM_ORDER_PLAIN
from test_hip_edges import gemm_bound

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
ARENA = None
FWD, BWD, NONE = _lib.NT_RIDER_SAMPLING_FWD, _lib.NT_RIDER_SAMPLING_BWD_WIN, _lib.NT_RIDER_NONE
PERSIST, ONE_ROUND = GEMM_NT_P8_224 | GEMM_NT_PERSIST, GEMM_NT_P8_224 | GEMM_NT_NO_PERSIST


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


# ---- inputs and float64 references, on the CPU (no device: tests/test_gemm_riders_host.py evaluates them in float32 too) ------------------------------
def windows_of(Hp, Wp):
    """(pad_t, pad_l, nh, nw) of RvsaWindows (csrc/common.h)"""
    ph, pw = (7 - Hp % 7) % 7, (7 - Wp % 7) % 7
    return ph // 2, pw // 2, (Hp + ph) // 7, (Wp + pw) // 7


@functools.lru_cache(maxsize=2)
def gemm_case(M, N, K, seed, bias=True):
    """a, w (bf16), bias (f32 or None), the float64 product with bias and its gemm_bound"""
    g = torch.Generator().manual_seed(seed)
    a, w, b = torch.randn(M, K, generator=g).to(BF16), (torch.randn(N, K, generator=g) * 0.1).to(BF16), torch.randn(N, generator=g)
    ref, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    if bias:
        ref, mag = ref + b.double(), mag + b.double().abs()
    return a, w, (b if bias else None), ref, gemm_bound(K, mag, ref, BF16)


def fwd_inputs(B, Hp, Wp, C, heads, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * Hp * Wp, C, generator=g).to(BF16), torch.randn(5 * heads, C, generator=g) * 0.05, torch.randn(5 * heads, generator=g)


def fwd_eval(x, ws, bs, B, Hp, Wp, dtype):
    """zero pad, AvgPool2d(7, 7), LeakyReLU(0.01), the stacked heads -- in `dtype`; also mean|x| per window and channel (float64)"""
    pt, pl_, nh, nw = windows_of(Hp, Wp)
    C = x.shape[1]
    xp = torch.zeros(B, nh * 7, nw * 7, C, dtype=dtype)
    xp[:, pt:pt + Hp, pl_:pl_ + Wp] = x.to(dtype).view(B, Hp, Wp, C)
    win = xp.view(B, nh, 7, nw, 7, C)
    avg = (win.sum(dim=(2, 4)) * torch.tensor(1.0 / 49.0, dtype=dtype)).reshape(B * nh * nw, C)
    pooled = torch.where(avg > 0, avg, torch.tensor(0.01, dtype=dtype) * avg)
    samp = pooled @ ws.to(dtype).t() + bs.to(dtype)
    mag = (win.abs().double().sum(dim=(2, 4)) / 49.0).reshape(B * nh * nw, C)
    return avg, pooled, samp, mag


@functools.lru_cache(maxsize=4)
def fwd_case(B, Hp, Wp, C, heads):
    """inputs, float64 references and the bounds of the module docstring"""
    x, ws, bs = fwd_inputs(B, Hp, Wp, C, heads)
    avg, pooled, samp, mag = fwd_eval(x, ws, bs, B, Hp, Wp, F64)
    avg_b = 2 * 49 * U * mag
    pooled_b = 2 * avg_b
    samp_b = 2 * C * U * (pooled.abs() @ ws.double().abs().t() + bs.double().abs()) + pooled_b @ ws.double().abs().t()
    return dict(x=x, ws=ws, bs=bs, avg=avg, pooled=pooled, samp=samp, avg_b=avg_b, pooled_b=pooled_b, samp_b=samp_b)


def bwd_inputs(R, C, N, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, N, generator=g), torch.randn(N, C, generator=g) * 0.05, torch.randn(R, C, generator=g)


def bwd_eval(dsamp, ws, avg, dtype):
    k = torch.tensor(1.0 / 49.0, dtype=dtype)
    return (dsamp.to(dtype) @ ws.to(dtype)) * torch.where(avg > 0, k, torch.tensor(0.01, dtype=dtype) * k)


@functools.lru_cache(maxsize=4)
def bwd_case(R, C, N):
    dsamp, ws, avg = bwd_inputs(R, C, N)
    fac = torch.where(avg > 0, torch.tensor(1.0 / 49.0, dtype=F64), torch.tensor(0.01 / 49.0, dtype=F64))
    return dict(dsamp=dsamp, ws=ws, avg=avg, g=bwd_eval(dsamp, ws, avg, F64), g_b=2 * N * U * (dsamp.double().abs() @ ws.double().abs()) * fac)


def worst(got, ref, bound, what):
    """max |got - ref| / bound, element-wise in float64; asserts it is at most 1 (a NaN -- a never-written element -- fails)"""
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    print("%s: worst |err| / bound = %.3g" % (what, ratio))
    assert ratio <= 1.0, "%s: %d of %d elements outside the bound, worst |err| / bound = %.3g" % (what, int((err > bound).sum() + err.isnan().sum()), err.numel(), ratio)
    return ratio


# ---- one case ---------------------------------------------------------------------------------------------------------------------------------------------
def device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def half_chip(ops):
    """(stream, its CU count): every second CU of every XCC"""
    words = ops.cu_mask_words("interleaved", 0)
    return ops.cu_mask_stream("cuda", words), sum(bin(w).count("1") for w in words)


def _on(stream, fn):
    if stream is None:
        return fn()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = fn()
    stream.synchronize()
    return out


def run_case(ops, name, gemm, variant, kind, sizes, expect, stream=None, cus=0, bias=True, gemm_seed=None, launches=3, values=True):
    """kind FWD: sizes = (B, Hp, Wp, C, heads); BWD: (windows, C, N); NONE: None.  expect: a function of the plan that asserts what the case exists for
    (it runs BEFORE anything is launched).  Returns the plan."""
    M, N, K = gemm
    a_, w_, b_, cref, cbound = gemm_case(M, N, K, gemm_seed if gemm_seed is not None else (3 if kind == BWD else 1), bias)
    a, w, b = dev(a_), dev(w_), (dev(b_) if bias else None)
    if kind == FWD:
        B, Hp, Wp, C, heads = sizes
        case = fwd_case(B, Hp, Wp, C, heads)
        x, ws, bs = dev(case["x"]), dev(case["ws"]), dev(case["bs"])
        _, _, nh, nw = windows_of(Hp, Wp)
        assert (nh, nw) == ops.rvsa_windows(Hp, Wp)
        R = B * nh * nw
        shapes = [(R, C), (R, C), (R, 5 * heads)]
        names = ["avg", "pooled", "samp"]
        make = lambda outs: ops.sampling_fwd_rider(x, ws, bs, outs[0], outs[1], outs[2], B, Hp, Wp)
        alone = lambda outs: ops.rvsa_sampling_fwd(x, ws, bs, outs[0], outs[1], outs[2], B, Hp, Wp)
    elif kind == BWD:
        R, C, Nh = sizes
        case = bwd_case(R, C, Nh)
        dsamp, ws, avg_in = dev(case["dsamp"]), dev(case["ws"]), dev(case["avg"])
        shapes, names = [(R, C)], ["g"]
        make = lambda outs: ops.sampling_bwd_win_rider(dsamp, ws, avg_in, outs[0])
        alone = lambda outs: ops.rvsa_sampling_bwd_win(dsamp, ws, avg_in, outs[0])
    else:
        case, shapes, names = {}, [], []
        make = lambda outs: _lib.NtRider(kind=NONE)
        alone = lambda outs: None
    # the decision, asserted before the first launch
    outs0, c0 = [e(*s) for s in shapes], e(M, N, dtype=BF16)
    plan = ops.gemm_nt_rider_plan(a, w, c0, make(outs0), bias=b, variant=variant, cus=cus)
    expect(plan)
    if plan.rides and kind != NONE:
        assert plan.gemm_wgs + plan.riders <= (cus or device_cus()) and plan.windows_per_rider == -(-shapes[0][0] // plan.riders)
    # what the launch replaces: the GEMM alone (this variant, and the 128-wide family), then the stand-alone kernel
    _on(stream, lambda: ops.gemm_nt(a, w, c0, bias=b, variant=variant))
    c128 = _on(stream, lambda: ops.gemm_nt(a, w, e(M, N, dtype=BF16), bias=b, variant=(variant & GEMM_ORDER_PLAIN) | GEMM_NT_NO_P8))
    _on(stream, lambda: alone(outs0))
    assert torch.equal(c0, c128), name + ": the P8 launch and the 128-wide family differ"
    for i in range(launches if plan.rides else 1):
        outs, c = [e(*s) for s in shapes], e(M, N, dtype=BF16)
        rider = make(outs)
        _on(stream, lambda: ops.gemm_nt(a, w, c, bias=b, variant=variant, rider=rider))
        assert torch.equal(c, c0), "%s: C differs from the launch without a rider (launch %d)" % (name, i)
        for n, got, ref in zip(names, outs, outs0):
            assert torch.equal(got, ref), "%s: %s differs from the stand-alone kernel (launch %d)" % (name, n, i)
    if values:
        record_parity("gemm_riders", name + " C", worst(c, cref, cbound, name + " C"))
        for n, got in zip(names, outs):
            record_parity("gemm_riders", name + " " + n, worst(got, case[n], case[n + "_b"], name + " " + n))
    return plan


def rides(**want):
    def check(plan):
        assert plan.rides == 1 and plan.reason == _lib.NT_RIDE_OK, (plan.rides, plan.reason)
        for k, v in want.items():
            assert getattr(plan, k) == v, (k, getattr(plan, k), v)
    return check


def falls_back(reason):
    def check(plan):
        assert plan.rides == 0 and plan.reason == reason, (plan.rides, plan.reason)
    return check


def _check_fwd(ops, gemm, sampler, variant, expect, stream=None, cus=0, name=None):
    return run_case(ops, name or "fwd %s %s" % (gemm, sampler), gemm, variant, FWD, sampler, expect, stream, cus)


def _check_bwd(ops, gemm, sampler, variant, expect, stream=None, cus=0, name=None):
    B, Hp, Wp, C, heads = sampler
    nh, nw = ops.rvsa_windows(Hp, Wp)
    return run_case(ops, name or "bwd %s %s" % (gemm, sampler), gemm, variant, BWD, (B * nh * nw, C, 5 * heads), expect, stream, cus)


# ---- the cases of the first rider tests: one tile per GEMM workgroup, at most two windows per rider ------------------------------------------------------
@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampling_forward_rides_the_persistent_gemm(ops, gemm, sampler):
    M, N, K = gemm
    a, w = gemm_case(M, N, K, 1)[:2]
    plan = ops.gemm_nt_plan(dev(a), dev(w), torch.empty(M, N, device="cuda", dtype=BF16), variant=PERSIST)
    assert (plan.family, plan.tile_m, plan.persistent, plan.store_policy) == (GEMM_NT_FAMILY_P8, 224, 1, 1)      # the instantiation that carries the rider
    assert ops.lib().mtp_nt_p8_gemm_wgs(2 * (N // 256), 256) == 2 * (N // 256)                                   # one round: spare CUs on any MI355X stream
    windows = sampler[0] * 4 if sampler[1] == 14 else sampler[0] * 6
    _check_fwd(ops, gemm, sampler, PERSIST, rides(gemm_wgs=2 * (N // 256), riders=min(32, windows)))


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_sampling_backward_factor_rides_the_one_round_gemm(ops, gemm, sampler):
    M, N, K = gemm
    a, w = gemm_case(M, N, K, 3)[:2]
    plan = ops.gemm_nt_plan(dev(a), dev(w), torch.empty(M, N, device="cuda", dtype=BF16), variant=ONE_ROUND)
    assert (plan.family, plan.tile_m, plan.persistent, plan.store_policy) == (GEMM_NT_FAMILY_P8, 224, 0, 1)
    windows = sampler[0] * 4 if sampler[1] == 14 else sampler[0] * 6
    _check_bwd(ops, gemm, sampler, ONE_ROUND, rides(gemm_wgs=2 * (N // 256), riders=min(32, windows)))


def test_no_spare_cu_falls_back_to_two_launches(ops):
    """a 128-CU stream and 128 tiles: every CU of the stream has a GEMM workgroup, nothing to lend"""
    st, scus = half_chip(ops)
    assert scus == 128 and ops.lib().mtp_nt_p8_gemm_wgs(128, 128) == 128
    _check_fwd(ops, (448, 16384, 128), SAMPLERS[1], PERSIST, falls_back(_lib.NT_RIDE_NO_SPARE_CU), stream=st, cus=scus)
    _check_bwd(ops, (448, 16384, 128), SAMPLERS[1], ONE_ROUND, falls_back(_lib.NT_RIDE_NO_SPARE_CU), stream=st, cus=scus)


def test_a_problem_the_p8_family_refuses_falls_back(ops):
    """K = 64 is half a K-tile pair: the 128-wide kernels run it, the rider's stand-alone kernel follows"""
    a, w = gemm_case(448, 512, 64, 1)[:2]
    assert ops.gemm_nt_plan(dev(a), dev(w), torch.empty(448, 512, device="cuda", dtype=BF16), variant=GEMM_NT_P8_224).family != GEMM_NT_FAMILY_P8
    _check_fwd(ops, (448, 512, 64), SAMPLERS[2], PERSIST, falls_back(_lib.NT_RIDE_NO_FAMILY))
    _check_bwd(ops, (448, 512, 64), SAMPLERS[2], ONE_ROUND, falls_back(_lib.NT_RIDE_NO_FAMILY))
    # the plan the other way round (a persistent launch under the backward rider, a one-round launch under the forward one): no instantiation, same results
    _check_fwd(ops, GEMMS[0], SAMPLERS[0], ONE_ROUND, falls_back(_lib.NT_RIDE_NO_INSTANTIATION))
    _check_bwd(ops, GEMMS[0], SAMPLERS[0], PERSIST, falls_back(_lib.NT_RIDE_NO_INSTANTIATION))


# ---- 1, 2: the persistent walk under riders takes a second and a third step (`tile += gemm_wgs`) ---------------------------------------------------------
def _walk_shape(steps, cus):
    """the smallest problems of 224 x 256 tiles and K = 128 whose walk on `cus` CUs has `steps` steps.  two: 448 rows (2 tile rows) and cus / 2 + 1 tile
    columns -- cus + 2 tiles.  three: 392 rows (224 + a ragged 168) and cus + 1 tile columns, the last one 72 wide -- 2 cus + 2 tiles"""
    return (448, 256 * (cus // 2 + 1), 128) if steps == 2 else (392, 256 * cus + 72, 128)


def _walks(steps, riders):
    def check(plan):
        rides(riders=riders)(plan)
        assert plan.gemm_wgs < check.ntiles and -(-check.ntiles // plan.gemm_wgs) == steps, (plan.gemm_wgs, check.ntiles)      # a workgroup with `steps` tiles
        assert (steps - 1) * plan.gemm_wgs < check.ntiles                                                            # ... and the stride is what takes it there
    return check


@pytest.mark.parametrize("kind", [FWD, NONE], ids=["fwd", "none"])
@pytest.mark.parametrize("order", [0, GEMM_ORDER_PLAIN], ids=["remap", "plain"])
@pytest.mark.parametrize("steps", [2, 3])
def test_persistent_walk_under_riders_takes_several_steps(ops, steps, order, kind):
    """more tiles than CUs on the whole chip: every GEMM workgroup walks `steps` tiles with the stride gemm_wgs, in both tile orders, with the forward rider
    (36 windows on 32 riders) and as the even walk alone (MTP_NT_RIDER_NONE).  The three-step shape has ragged last tiles in M and N."""
    cus = device_cus()
    M, N, K = gemm = _walk_shape(steps, cus)
    check = _walks(steps, 32 if kind == FWD else 0)
    check.ntiles = -(-M // 224) * -(-N // 256)
    assert check.ntiles > cus
    run_case(ops, "walk %d steps order %d kind %d" % (steps, order, kind), gemm, PERSIST | order, kind, SAMPLERS[1] if kind == FWD else None, check, gemm_seed=5)


def test_persistent_walk_on_a_masked_half_chip_stream(ops):
    """a 128-CU stream and 130 tiles: 65 workgroups walk two tiles each, 63 CUs are spare, 32 riders"""
    st, scus = half_chip(ops)
    M, N, K = gemm = _walk_shape(2, scus)
    check = _walks(2, 32)
    check.ntiles = 2 * (N // 256)
    plan = run_case(ops, "walk half chip", gemm, PERSIST, FWD, SAMPLERS[1], check, stream=st, cus=scus, gemm_seed=5)
    assert scus - plan.gemm_wgs >= 32 and plan.gemm_wgs == scus // 2 + 1


# ---- 3, 4: the trip counts of the rider loops -----------------------------------------------------------------------------------------------------------------
# (B, Hp, Wp, C, heads) -> windows per rider on 32 riders.  256 windows: 8 -- the step's count: 4 pool iterations, 2 rounds of head passes, 4 backward
# iterations.  160: 5 -- odd (the dead second half of the last pool iteration pools a clamped window into row 5) and no multiple of 4 (the second round of
# head passes has one live row; rows 6 and 7 of the LDS were never written).  15 x 10 tokens: 3 x 2 windows that hang over the edge, 96 of them: 3
TRIPS = [((64, 14, 14, 128, 2), 8), ((40, 14, 14, 128, 2), 5), ((16, 15, 10, 128, 2), 3)]


@pytest.mark.parametrize("sampler,per", TRIPS)
def test_forward_rider_trip_counts(ops, sampler, per):
    _check_fwd(ops, GEMMS[0], sampler, PERSIST, rides(gemm_wgs=4, riders=32, windows_per_rider=per, scratch_bytes=-(-per // 4) * 4 * 4 * 128))


@pytest.mark.parametrize("sampler,per", TRIPS)
def test_backward_rider_trip_counts(ops, sampler, per):
    _check_bwd(ops, GEMMS[0], sampler, ONE_ROUND, rides(gemm_wgs=4, riders=32, windows_per_rider=per))


@pytest.mark.parametrize("spare,per", [(1, 36), (8, 5)])
def test_few_riders_long_loops(ops, spare, per):
    """a 128-CU stream whose GEMM takes all but `spare` CUs (one tile row, 128 - spare tile columns): 36 windows on one rider (18 pool and backward iterations,
    9 rounds of head passes) and on 8 riders (5 each)"""
    st, scus = half_chip(ops)
    gemm = (224, 256 * (scus - spare), 128)
    want = dict(gemm_wgs=scus - spare, riders=spare, windows_per_rider=per)
    _check_fwd(ops, gemm, SAMPLERS[1], PERSIST, rides(**want), stream=st, cus=scus, name="few riders fwd spare %d" % spare)
    _check_bwd(ops, gemm, SAMPLERS[1], ONE_ROUND, rides(**want), stream=st, cus=scus, name="few riders bwd spare %d" % spare)


# ---- 5, 6: the widths of the models ------------------------------------------------------------------------------------------------------------------------------
# (C, heads): ViT-L (all four k-slices of a lane live, 80 outputs: 20 column passes on 8 waves), ViT-B (the fourth slice masked, 60 outputs), 1280 channels
# (a second k0 iteration with a masked tail; 15 outputs: the last pass of wave 3 is partly masked, waves 4 .. 7 have none)
@pytest.mark.parametrize("C,heads", [(1024, 16), (768, 12), (1280, 3)])
def test_forward_rider_at_model_widths(ops, C, heads):
    _check_fwd(ops, GEMMS[0], (3, 14, 14, C, heads), PERSIST, rides(gemm_wgs=4, riders=12, windows_per_rider=1, scratch_bytes=4 * 4 * C))


def test_forward_rider_at_the_scratch_limit(ops):
    """C = 8192, the widest the entry point takes, on 8 riders (a 128-CU stream, 120 tiles): 32 windows are 4 pooled rows of 32 KiB per rider -- 128 KiB, it
    rides; 36 windows are 5, kept in whole groups of 4: 256 KiB against the launch's 160 -- refused, and the two launches give the same results"""
    st, scus = half_chip(ops)
    gemm = (224, 256 * (scus - 8), 128)
    _check_fwd(ops, gemm, (8, 14, 14, 8192, 2), PERSIST, rides(riders=8, windows_per_rider=4, scratch_bytes=128 * 1024), stream=st, cus=scus, name="fwd C 8192 rows 4")

    def refused(plan):
        falls_back(_lib.NT_RIDE_NO_SCRATCH)(plan)
        assert (plan.riders, plan.windows_per_rider, plan.scratch_bytes) == (8, 5, 256 * 1024)
    _check_fwd(ops, gemm, (9, 14, 14, 8192, 2), PERSIST, refused, stream=st, cus=scus, name="fwd C 8192 rows 8 refused")


# (windows, C, N): ViT-L (4 channel-quad blocks of 64 per window, 20 head outputs per wave); 1280 channels (5 blocks); N = 5 (2 outputs per wave: wave 2 has
# one, wave 3 an empty range); N = 4096, the most the entry point takes (16 KiB of dsamp per half)
@pytest.mark.parametrize("R,C,N", [(12, 1024, 80), (12, 1280, 15), (12, 128, 5), (12, 128, 4096)])
def test_backward_rider_at_model_widths(ops, R, C, N):
    run_case(ops, "bwd widths %s" % ((R, C, N),), GEMMS[0], ONE_ROUND, BWD, (R, C, N),
             rides(gemm_wgs=4, riders=12, windows_per_rider=1, scratch_bytes=2 * (4096 + (4 * N + 15) // 16 * 16)))


# ---- 7: the GEMM without a bias, as the engine launches the backward one ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [FWD, BWD], ids=["fwd", "bwd"])
def test_riders_under_a_gemm_without_bias(ops, kind):
    if kind == FWD:
        run_case(ops, "no bias fwd", GEMMS[1], PERSIST, FWD, SAMPLERS[1], rides(gemm_wgs=6, riders=32, windows_per_rider=2), bias=False)
    else:
        run_case(ops, "no bias bwd", GEMMS[1], ONE_ROUND, BWD, (36, 128, 10), rides(gemm_wgs=6, riders=32, windows_per_rider=2), bias=False)
