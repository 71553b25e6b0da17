"""GPU: the RVSA sampling heads (csrc/rvsa_sampling.hip, csrc/rvsa_sampling_body.h) on the edge grids, at the widths and head counts where their kernels
change path, and in the LeakyReLU-kink and non-finite regimes -- every buffer out of the guard arena (tests/guard.py): outputs NaN-poisoned and between
guards, inputs frozen.  Every output goes through Arena.check_written before it is compared (the helpers within / same call it).

The cases and the float64 references are tests/sampling_cases.py.  The element-wise bound is the project's,

    |got - ref| <= 2 T 2^-24 sum|terms|   [+ 2^-8 |ref| for a bf16 output]

with T = 50 for avg (49 adds and the 1 / 49 scaling), 52 for pooled, K + 1 for samp and small_linear_fwd (K = C, plus the bias), N for small_linear's dx,
R for dw / db, N + 2 for the per-window addend g, N + 3 for rvsa_sampling_bwd's dx and 3 for rvsa_pool_bwd's.  The reference of samp is computed from
the device's own pooled rows, read back: that keeps the product apart from the pooling error, which has its own bound.  Where the inputs are small
integers every f32 sum is an integer below 2^24 and the result is compared with torch.equal, whatever the order of the atomics.

tests/test_sampling_edges_host.py asserts on the CPU, for these very inputs, that a float32 evaluation stays within half of each bound, that every avg
element is decided exactly or KINK away from 0, that every named seam value lands on its branch, and that the exact-sum inputs stay below 2^24."""
import ctypes as C

import pytest
import torch

import guard
import sampling_cases as S

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
DTID = ["f32", "bf16"]
ARENA = None     # the running test's guard.Arena
ERR_ARG = r"^%s failed: invalid argument$"      # what _lib.check raises for MTP_ERR_ARG (-1) and for nothing else
CASES = S.sampling_cases()


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
    try:
        a.check()
    finally:
        a.close()


def dev(t, dtype=None):
    """an op INPUT: guarded and frozen (None stays None)"""
    return None if t is None else ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t, dtype=None):
    """updated in place by contract: guarded, not frozen"""
    return ARENA.like(t, dtype=dtype or t.dtype)


def e(*shape, dtype=F32):
    """an op OUTPUT: NaN-poisoned, between guards"""
    return ARENA.empty(*shape, dtype=dtype)


def written(t, what=""):
    ARENA.check_written(t, what or None)
    return t


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()]).cpu()


def same(got, want, what=""):
    """written in full and equal in value to `want` (a CPU tensor), element for element"""
    written(got, what)
    g = got.cpu()
    assert torch.equal(g.float(), want.float().reshape(g.shape)), "%s: %d of %d elements differ" % (what, int((g.float() != want.float().reshape(g.shape)).sum()), g.numel())


def same_bits(a, b, what=""):
    """two device outputs, bit for bit (NaN included)"""
    assert torch.equal(bits(a), bits(b)), "%s: %d elements differ in their bits" % (what, int((bits(a) != bits(b)).sum()))


def within(got, ref, bound, what=""):
    """element-wise |got - ref| <= bound, all in float64; the device output is first checked to be written in full"""
    written(got, what)
    got, ref = got.double().cpu().reshape(ref.shape), ref.double()
    err = (got - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), "%s: %d of %d elements outside the bound; worst |err| / bound = %.3g at %s" % (
        what, int((~ok).sum()), ok.numel(), float((err / bound.clamp_min(1e-300))[~ok].nan_to_num(float("inf")).max()), tuple((~ok).nonzero()[0].tolist()))


def st():
    return torch.cuda.current_stream().cuda_stream


def refused(ops, name, *args):
    with pytest.raises(RuntimeError, match=ERR_ARG % name):
        ops.check(getattr(ops.lib(), name)(*args), name)


def forward(ops, c, case, dtype, x=None, fused=True):
    """(avg, pooled, samp) of rvsa_sampling_fwd, or (avg, pooled) of rvsa_pool_fwd, into fresh poisoned outputs"""
    Hp, Wp, B, Cc, N, _ = case
    x = dev(c["x"] if x is None else x, dtype)
    avg, pooled = e(c["R"], Cc), e(c["R"], Cc)
    if not fused:
        ops.rvsa_pool_fwd(x, avg, pooled, B, Hp, Wp)
        return avg, pooled
    samp = e(c["R"], N)
    ops.rvsa_sampling_fwd(x, dev(c["w"]), dev(c["b"]), avg, pooled, samp, B, Hp, Wp)
    return avg, pooled, samp


# ================================================================================================ 1. forward
def check_forward(ops, case, dtype):
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    avg0, pooled0 = forward(ops, c, case, dtype, fused=False)
    avg, pooled, samp = forward(ops, c, case, dtype)
    within(avg0, c["avg"], S.sum_bound(S.TERMS["avg"](Cc, N), c["avgmag"], c["avg"]), "rvsa_pool_fwd avg")
    within(pooled0, c["pooled"], S.sum_bound(S.TERMS["pooled"](Cc, N), c["pooledmag"], c["pooled"]), "rvsa_pool_fwd pooled")
    written(avg, "fused avg"), written(pooled, "fused pooled")
    same_bits(avg, avg0, "fused avg against rvsa_pool_fwd")
    same_bits(pooled, pooled0, "fused pooled against rvsa_pool_fwd")
    ref, mag = S.samp_ref(pooled.cpu(), c["w"], c["b"])
    within(samp, ref, S.sum_bound(S.TERMS["samp"](Cc, N), mag, ref), "samp")
    # the constructed window-channels: their sign is decided exactly, and so is every bit of them
    same(avg0[0, :S.MADE], c["avg_made"], "constructed avg")
    same(pooled0[0, :S.MADE], c["pooled_made"], "constructed pooled")
    assert bool((pooled0[0, [0, 3]] == 0).all())
    for a, b, name in zip(forward(ops, c, case, dtype), (avg, pooled, samp), ("avg", "pooled", "samp")):
        same_bits(written(a), b, "second call, " + name)


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_forward_bounds_fused_equals_separate_and_repeats(ops, case, dtype):
    check_forward(ops, case, dtype)


@pytest.mark.parametrize("N", [32, 33, 60, 83])
def test_head_outputs_do_not_depend_on_the_workgroup_that_makes_them(ops, N):
    """N >= 32: two workgroups per window, each with its share of the outputs.  The same heads 30 at a time -- one workgroup per window, other passes, other
    waves, slices that straddle the two shares -- give the same bits.  (Slices start on an even head: rvsa_heads rounds the x product first in the even
    columns of a pass and the y product in the odd ones, and a share starts on a multiple of four.)"""
    case = (8, 8, 3, 1028, N, True)
    Hp, Wp, B, Cc, _, _ = case
    c = S.sampling_case(*case)
    x, R = dev(c["x"]), c["R"]
    avg, pooled, samp = forward(ops, c, case, F32)
    written(samp)
    for lo in range(0, N, 30):
        hi = min(lo + 30, N)
        part = e(R, hi - lo)
        ops.rvsa_sampling_fwd(x, dev(c["w"][lo:hi].contiguous()), dev(c["b"][lo:hi].contiguous()), e(R, Cc), e(R, Cc), part, B, Hp, Wp)
        same_bits(written(part), samp[:, lo:hi], "heads [%d, %d)" % (lo, hi))


def test_forward_at_the_widest_row_it_accepts(ops):
    """C = 8192 (the pooled row's 32 KB of LDS), one window"""
    check_forward(ops, (1, 1, 1, S.C_MAX, 5, True), F32)


# ================================================================================================ 2. backward
def kernel_factor(avg):
    """what the three backward kernels multiply with, in float32 as they do: 1 / 49 where avg > 0, else 0.01f * (1 / 49)"""
    k = torch.tensor(1.0) / torch.tensor(49.0)
    return torch.where(avg > 0, k, torch.tensor(0.01) * k)


def check_backward(ops, case, dtype):
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    R, T, tw = c["R"], c["T"], c["tw"]
    dsamp, w, avg, dp = dev(c["dsamp"]), dev(c["w"]), dev(c["avg_in"]), dev(c["dpooled"])
    base = c["base"].double()
    g = ops.rvsa_sampling_bwd_win(dsamp, w, avg, e(R, Cc))
    within(g, c["g"], S.sum_bound(S.TERMS["g"](Cc, N), c["gmag"], c["g"]), "g")
    dx = io(c["base"], dtype)
    ops.rvsa_sampling_bwd(dsamp, w, avg, dx, B, Hp, Wp)
    ref = base + c["g"][tw]
    within(dx, ref, S.sum_bound(S.TERMS["sampling_dx"](Cc, N), base.abs() + c["gmag"][tw], ref, dtype), "rvsa_sampling_bwd dx")
    T3 = S.TERMS["pool_dx"](Cc, N)
    out = e(T, Cc, dtype=dtype)
    ops.rvsa_pool_bwd(dp, avg, out, B, Hp, Wp, accumulate=False)
    ref = c["pg"][tw]
    within(out, ref, S.sum_bound(T3, ref.abs(), ref, dtype), "rvsa_pool_bwd dx")
    acc = io(c["base"], dtype)
    ops.rvsa_pool_bwd(dp, avg, acc, B, Hp, Wp, accumulate=True)
    ref = base + c["pg"][tw]
    within(acc, ref, S.sum_bound(T3, base.abs() + c["pg"][tw].abs(), ref, dtype), "rvsa_pool_bwd dx +=")
    if dtype == F32:
        # onto zeros rvsa_sampling_bwd leaves exactly the g of each token's window; rvsa_pool_bwd's product is one f32 multiplication
        zero = ARENA.zeros(T, Cc)
        ops.rvsa_sampling_bwd(dsamp, w, avg, zero, B, Hp, Wp)
        same(zero, g.cpu()[tw], "rvsa_sampling_bwd onto zeros against rvsa_sampling_bwd_win")
        same(out, (c["dpooled"] * kernel_factor(c["avg_in"]))[tw], "rvsa_pool_bwd, exact product")


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_backward_against_the_float64_adjoint(ops, case, dtype):
    check_backward(ops, case, dtype)


def test_backward_at_the_most_heads_it_accepts(ops):
    """N = 4096 (the dsamp row's 16 KB of LDS) in rvsa_sampling_bwd and rvsa_sampling_bwd_win"""
    check_backward(ops, (1, 1, 1, 4, S.N_MAX, True), F32)


@pytest.mark.parametrize("case", [(8, 8, 1, 260, 33, True), (1, 1, 3, 4, 5, True)], ids=S.case_id)
def test_slopes_at_the_kink_are_exact(ops, case):
    """integer dsamp and w: dsamp . w is exact, so g is ONE rounded product with 1 / 49 (avg > 0) or 0.01f / 49 (avg <= 0: at 0.0 and -0.0 the slope is 0.01,
    as in torch's LeakyReLU backward) -- every element is compared exactly, the constructed ones (0.0, -0.0, +-2^-20 / 49) among them"""
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    R, T, tw = c["R"], c["T"], c["tw"]
    ds, w = S.ints(R, N, seed=1), S.ints(N, Cc, seed=2)
    fac = kernel_factor(c["avg_in"])
    k = float(torch.tensor(1.0) / torch.tensor(49.0))
    assert fac[0, :S.MADE].tolist() == [float(torch.tensor(0.01) * k)] * 2 + [k] + [float(torch.tensor(0.01) * k)]
    want = (ds.double() @ w.double()).float() * fac
    dsamp, wd, avg = dev(ds), dev(w), dev(c["avg_in"])
    same(ops.rvsa_sampling_bwd_win(dsamp, wd, avg, e(R, Cc)), want, "g")
    zero = ARENA.zeros(T, Cc)
    ops.rvsa_sampling_bwd(dsamp, wd, avg, zero, B, Hp, Wp)
    same(zero, want[tw], "rvsa_sampling_bwd onto zeros")


# ================================================================================================ 3. isolation
ISO = [(8, 8, 3, 1028, 33, True), (6, 15, 3, 1024, 83, True)]


def rows_of(c, B, image):
    per = c["R"] // B
    return slice(image * per, (image + 1) * per)


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("case", ISO, ids=S.case_id)
def test_forward_windows_see_only_their_own_tokens(ops, case, dtype):
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    tw, per = c["tw"], Hp * Wp
    a = [written(t) for t in forward(ops, c, case, dtype)]
    # image 1 replaced: the windows of images 0 and 2 keep their bits, those of image 1 change
    x1 = c["x"].clone()
    x1[per:2 * per] = S.tokens(Hp, Wp, 1, Cc, seed=77)
    b = [written(t) for t in forward(ops, c, case, dtype, x=x1)]
    for u, v, name in zip(a, b, ("avg", "pooled", "samp")):
        for image in (0, 2):
            same_bits(u[rows_of(c, B, image)], v[rows_of(c, B, image)], "%s of image %d" % (name, image))
        assert not torch.equal(bits(u[rows_of(c, B, 1)]), bits(v[rows_of(c, B, 1)])), name
    # one token replaced (the last of image 0, a pad-side window): only its own window's rows change
    t = per - 1
    x2 = c["x"].clone()
    x2[t] = x2[t] + 1.0
    b = [written(t_) for t_ in forward(ops, c, case, dtype, x=x2)]
    own = int(tw[t])
    for u, v, name in zip(a, b, ("avg", "pooled", "samp")):
        changed = (bits(u) != bits(v)).any(1).nonzero().reshape(-1).tolist()
        assert changed == [own], "%s: rows %s changed, the token's window is %d" % (name, changed, own)
    for u, v in zip(forward(ops, c, case, dtype, x=x2, fused=False), b[:2]):
        same_bits(written(u), v)


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("case", ISO, ids=S.case_id)
def test_backward_tokens_see_only_their_own_window(ops, case, dtype):
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    R, T, tw, per, wper = c["R"], c["T"], c["tw"], Hp * Wp, c["R"] // B

    def run(dsamp, dpooled, avg_in, base):
        ds, w, avg, dp = dev(dsamp), dev(c["w"]), dev(avg_in), dev(dpooled)
        g = ops.rvsa_sampling_bwd_win(ds, w, avg, e(R, Cc))
        dx = io(base, dtype)
        ops.rvsa_sampling_bwd(ds, w, avg, dx, B, Hp, Wp)
        acc = io(base, dtype)
        ops.rvsa_pool_bwd(dp, avg, acc, B, Hp, Wp, accumulate=True)
        out = e(T, Cc, dtype=dtype)
        ops.rvsa_pool_bwd(dp, avg, out, B, Hp, Wp, accumulate=False)
        return [written(g), written(dx), written(acc), written(out)]

    a = run(c["dsamp"], c["dpooled"], c["avg_in"], c["base"])
    # everything of image 1 replaced: its windows' dsamp, dpooled and avg rows, and its tokens' starting values
    ds1, dp1, av1, ba1 = c["dsamp"].clone(), c["dpooled"].clone(), c["avg_in"].clone(), c["base"].clone()
    ds1[wper:2 * wper], dp1[wper:2 * wper] = S.rnd(wper, N, seed=5), S.rnd(wper, Cc, seed=6)
    av1[wper:2 * wper], ba1[per:2 * per] = -av1[wper:2 * wper], S.rnd(per, Cc, seed=7)
    b = run(ds1, dp1, av1, ba1)
    for u, v, n in zip(a, b, (wper, per, per, per)):
        same_bits(u[:n], v[:n], "image 0")
        same_bits(u[2 * n:], v[2 * n:], "image 2")
        assert not torch.equal(bits(u[n:2 * n]), bits(v[n:2 * n]))
    # one window's rows replaced (the last of image 0): only its tokens change
    own = wper - 1
    ds2, dp2 = c["dsamp"].clone(), c["dpooled"].clone()
    ds2[own], dp2[own] = ds2[own] + 1.0, dp2[own] + 1.0
    b = run(ds2, dp2, c["avg_in"], c["base"])
    changed = (bits(a[0]) != bits(b[0])).any(1).nonzero().reshape(-1).tolist()
    assert changed == [own]
    mine = (tw == own)
    for u, v in zip(a[1:], b[1:]):
        ch = (bits(u) != bits(v)).any(1)
        assert not bool(ch[~mine].any()) and bool(ch[mine].all())


# ================================================================================================ 4. the non-finite regime
@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("fused", [False, True], ids=["pool_fwd", "sampling_fwd"])
@pytest.mark.parametrize("case", [(8, 8, 3, 1028, 33, True), (1, 13, 3, 4, 32, True)], ids=S.case_id)
def test_an_infinite_token_stays_in_its_own_window(ops, case, fused, dtype):
    """token (0, 0) of image 1 is +Inf.  On 8 x 8 the bottom window row and the right window column reach row 0 / column 0 only as padding; on 1 x 13 the right
    window does.  Every window but the token's own keeps its bits; the token's own window is non-finite in every output."""
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    t = Hp * Wp                                   # token (0, 0) of image 1
    own = int(c["tw"][t])
    x = c["x"].clone()
    x[t] = float("inf")
    a = forward(ops, c, case, dtype, fused=fused)
    b = forward(ops, c, case, dtype, x=x, fused=fused)
    others = torch.arange(c["R"]) != own
    for u, v, name in zip(a, b, ("avg", "pooled", "samp")):
        written(u, name), written(v, name)
        diff = (bits(u) != bits(v)).any(1)
        assert not bool(diff[others].any()), "%s: windows %s changed, the token is in window %d" % (name, diff.nonzero().reshape(-1).tolist(), own)
        assert not bool(torch.isfinite(v[own]).any()), name


# ================================================================================================ 5. / 6. small_linear
def check_sum(got, ref, mag, T, exact, what):
    if exact:
        same(got, ref.float(), what)
    else:
        within(got, ref, S.sum_bound(T, mag, ref), what)


@pytest.mark.parametrize("exact", [True, False], ids=["ints", "real"])
@pytest.mark.parametrize("R,N,K", S.small_linear_cases())
def test_small_linear_forward_and_backward(ops, R, N, K, exact):
    c = S.linear_case(R, N, K, exact)
    x, w, b, dy = dev(c["x"]), dev(c["w"]), dev(c["b"]), dev(c["dy"])
    check_sum(ops.small_linear_fwd(x, w, b, e(R, N)), c["y"], c["ymag"], K + 1, exact, "y")
    dx, dw, db = e(R, K), e(N, K), e(N)
    ops.small_linear_bwd(x, w, dy, dx, dw, db)
    check_sum(dx, c["dx"], c["dxmag"], N, exact, "dx")
    check_sum(dw, c["dw"], c["dwmag"], R, exact, "dw")
    check_sum(db, c["db"], c["dbmag"], R, exact, "db")


@pytest.mark.parametrize("form", ["no_bias", "no_dx", "no_db", "one_buffer", "dx_only"])
@pytest.mark.parametrize("R,N,K", [(5, 9, 2048), (129, 83, 1028), (33, 7, 2052)])
def test_small_linear_optional_outputs(ops, R, N, K, form):
    """bias = NULL; dx = NULL; db = NULL; [dw | db] as one buffer (db == dw + N K: one clearing pass); dw = NULL.  What is not passed is not written:
    the arena's guards see it."""
    c = S.linear_case(R, N, K, True)
    x, w, dy = dev(c["x"]), dev(c["w"]), dev(c["dy"])
    if form == "no_bias":
        return same(ops.small_linear_fwd(x, w, None, e(R, N)), c["y0"], "y")
    dx = None if form == "no_dx" else e(R, K)
    if form == "one_buffer":
        buf = e(N * K + N)
        dw, db = buf[:N * K].view(N, K), buf[N * K:]
        assert db.data_ptr() == dw.data_ptr() + 4 * N * K
    else:
        buf, dw, db = None, (None if form == "dx_only" else e(N, K)), (e(N) if form in ("no_dx",) else None)
    ops.small_linear_bwd(x, w, dy, dx, dw, db)
    if buf is not None:
        written(buf, "[dw | db]")
    for got, name in ((dx, "dx"), (dw, "dw"), (db, "db")):
        if got is not None:
            same(got, c[name], name)


def test_small_linear_dx_at_the_last_row_count_its_grid_takes(ops):
    """R = 4 * 65535: grid.y of small_linear_dx is 65535, the most a launch takes (one more row is refused, below); integers, dw summed over 2048 workgroups"""
    R, N, K = S.DX_ROWS_MAX, 1, 4
    c = S.linear_case(R, N, K, True)
    dx, dw, db = e(R, K), e(N, K), e(N)
    ops.small_linear_bwd(dev(c["x"]), dev(c["w"]), dev(c["dy"]), dx, dw, db)
    same(dx, c["dx"], "dx"), same(dw, c["dw"], "dw"), same(db, c["db"], "db")


# ================================================================================================ 7. segments
def check_segments(c, rows, bw, bb, gw, gb, R, exact, what=""):
    r0 = 0
    for j, r in enumerate(rows):
        sl = slice(r0, r0 + r)
        check_sum(gw[j], bw[j].double() + c["dw"][sl], bw[j].double().abs() + c["dwmag"][sl], R, exact, "%sdw[%d]" % (what, j))
        if gb[j] is not None:
            check_sum(gb[j], bb[j].double() + c["db"][sl], bb[j].double().abs() + c["dbmag"][sl], R, exact, "%sdb[%d]" % (what, j))
        r0 += r


@pytest.mark.parametrize("exact", [True, False], ids=["ints", "real"])
@pytest.mark.parametrize("R,K,rows,has_db", S.segment_cases(), ids=S.case_id)
def test_dw_segments_accumulate_into_their_parameters(ops, R, K, rows, has_db, exact):
    """every segment is its own guarded buffer holding starting values: a row that lands in the neighbouring segment, or a db written where none was
    passed, is seen; the sums are added to what was there"""
    N = sum(rows)
    c = S.linear_case(R, N, K, exact)
    bw, bb = S.seg_buffers(rows, has_db, K, exact)
    gw, gb = [io(t) for t in bw], [None if t is None else io(t) for t in bb]
    ops.small_linear_dw_segments(dev(c["x"]), dev(c["dy"]), gw, gb)
    check_segments(c, rows, bw, bb, gw, gb, R, exact)


def test_dw_segments_without_any_db(ops):
    """db = NULL for the whole call"""
    R, K, rows = 33, 260, (3, 5, 1, 2)
    N, n = sum(rows), len(rows)
    c = S.linear_case(R, N, K, True)
    bw, _ = S.seg_buffers(rows, (False,) * n, K, True)
    gw = [io(t) for t in bw]
    P = C.c_void_p * n
    ops.check(ops.lib().mtp_small_linear_dw_segments(dev(c["x"]).data_ptr(), dev(c["dy"]).data_ptr(), R, N, K, n, (C.c_int64 * n)(*rows),
                                                     P(*[t.data_ptr() for t in gw]), None, st()), "mtp_small_linear_dw_segments")
    check_segments(c, rows, bw, [None] * n, gw, [None] * n, R, True)


@pytest.mark.parametrize("count,exact", [(1, True), (S.SL_BATCH, True), (S.SL_BATCH, False)], ids=["1-ints", "8-ints", "8-real"])
def test_batched_dw_segments_equal_their_unbatched_calls(ops, count, exact):
    """R = 129: blockIdx.z = problem * 2 + row part, the last part one row long.  Integers: every problem equals the int64 product and, bit for bit, its own
    unbatched call.  Real values (the two row parts of a problem meet in atomics, in either order): every problem within the sum bound."""
    R, rows = S.BATCHED["R"], S.BATCHED["rows"]
    jobs, kept = [], []
    for i in range(count):
        c, (bw, bb) = S.batched_problem(i, exact)
        x, dy = dev(c["x"]), dev(c["dy"])
        gw, gb = [io(t) for t in bw], [None if t is None else io(t) for t in bb]
        uw, ub = [io(t) for t in bw], [None if t is None else io(t) for t in bb]
        ops.small_linear_dw_segments(x, dy, uw, ub)
        jobs.append((x, dy, gw, gb))
        kept.append((c, bw, bb, gw, gb, uw, ub))
    ops.small_linear_dw_segments_flush(jobs)
    for i, (c, bw, bb, gw, gb, uw, ub) in enumerate(kept):
        check_segments(c, rows, bw, bb, gw, gb, R, exact, "problem %d: " % i)
        for a, b in zip(gw + gb, uw + ub):
            if a is not None and exact:
                same_bits(a, b, "problem %d against its unbatched call" % i)


# ================================================================================================ 8. refusals
def test_pool_and_sampling_entry_points_refuse_without_writing(ops):
    """C off four, a size of 0, C = 8196 (forward), N = 4097 (backward), a NULL among the required pointers: MTP_ERR_ARG, and every output keeps its poison"""
    B, Hp, Wp, Cc, N = 1, 8, 8, 8, 4
    T, R = B * Hp * Wp, 4
    x, w, bias, avg_in, ds, dp = dev(S.rnd(T, Cc)), dev(S.rnd(N, Cc)), dev(S.rnd(N)), dev(S.rnd(R, Cc)), dev(S.rnd(R, N)), dev(S.rnd(R, Cc))
    avg, pooled, samp, g, dx = ARENA.wide(R, Cc), ARENA.wide(R, Cc), ARENA.wide(R, N), ARENA.wide(R, Cc), ARENA.wide(T, Cc)      # no column registered: all poison
    p = lambda t: t.data_ptr()
    dt = ops.MTP_F32
    sizes = [(B, Hp, Wp, 6), (0, Hp, Wp, Cc), (B, 0, Wp, Cc), (B, Hp, 0, Cc), (B, Hp, Wp, 0), (B, -1, Wp, Cc)]
    for s in sizes:
        refused(ops, "mtp_rvsa_pool_fwd", p(x), dt, p(avg), p(pooled), *s, st())
        refused(ops, "mtp_rvsa_pool_bwd", p(dp), p(avg_in), p(dx), dt, 0, *s, st())
        refused(ops, "mtp_rvsa_sampling_fwd", p(x), dt, p(w), p(bias), p(avg), p(pooled), p(samp), *s, N, st())
        refused(ops, "mtp_rvsa_sampling_bwd", p(ds), p(w), p(avg_in), p(dx), dt, *s, N, st())
    refused(ops, "mtp_rvsa_sampling_fwd", p(x), dt, p(w), p(bias), p(avg), p(pooled), p(samp), B, Hp, Wp, Cc, 0, st())
    refused(ops, "mtp_rvsa_sampling_bwd", p(ds), p(w), p(avg_in), p(dx), dt, B, Hp, Wp, Cc, 0, st())
    for s in [(0, Cc, N), (R, 0, N), (R, 6, N), (R, Cc, 0)]:
        refused(ops, "mtp_rvsa_sampling_bwd_win", p(ds), p(w), p(avg_in), p(g), *s, st())
    for i in range(3):
        a = [p(x), p(avg), p(pooled)]
        a[i] = None
        refused(ops, "mtp_rvsa_pool_fwd", a[0], dt, a[1], a[2], B, Hp, Wp, Cc, st())
        a = [p(dp), p(avg_in), p(dx)]
        a[i] = None
        refused(ops, "mtp_rvsa_pool_bwd", a[0], a[1], a[2], dt, 0, B, Hp, Wp, Cc, st())
    for i in range(5):
        a = [p(x), p(w), p(avg), p(pooled), p(samp)]
        a[i] = None
        refused(ops, "mtp_rvsa_sampling_fwd", a[0], dt, a[1], p(bias), a[2], a[3], a[4], B, Hp, Wp, Cc, N, st())
    for i in range(4):
        a = [p(ds), p(w), p(avg_in), p(dx)]
        a[i] = None
        refused(ops, "mtp_rvsa_sampling_bwd", a[0], a[1], a[2], a[3], dt, B, Hp, Wp, Cc, N, st())
        a = [p(ds), p(w), p(avg_in), p(g)]
        a[i] = None
        refused(ops, "mtp_rvsa_sampling_bwd_win", a[0], a[1], a[2], a[3], R, Cc, N, st())
    # one more than the largest accepted, with buffers of that size
    Cw = S.C_MAX + 4
    xw, ww, aw, pw, sw = dev(S.rnd(1, Cw)), dev(S.rnd(N, Cw)), ARENA.wide(1, Cw), ARENA.wide(1, Cw), ARENA.wide(1, N)
    refused(ops, "mtp_rvsa_sampling_fwd", p(xw), dt, p(ww), p(bias), p(aw), p(pw), p(sw), 1, 1, 1, Cw, N, st())
    Nw = S.N_MAX + 1
    dsw, wn, an, dxn, gn = dev(S.rnd(1, Nw)), dev(S.rnd(Nw, 4)), dev(S.rnd(1, 4)), ARENA.wide(1, 4), ARENA.wide(1, 4)
    refused(ops, "mtp_rvsa_sampling_bwd", p(dsw), p(wn), p(an), p(dxn), dt, 1, 1, 1, 4, Nw, st())
    refused(ops, "mtp_rvsa_sampling_bwd_win", p(dsw), p(wn), p(an), p(gn), 1, 4, Nw, st())
    torch.cuda.synchronize()
    ARENA.check()


def test_small_linear_entry_points_refuse_without_writing(ops):
    """R, N or K of 0, K off four, nseg of 0 and 5, segment rows that do not sum to N, count 0 and 9, a row count whose dx grid exceeds 65535 in y, a NULL
    among the required pointers: MTP_ERR_ARG, and every output keeps its poison"""
    R, N, K = 5, 8, 8
    x, w, b, dy = dev(S.rnd(R, K)), dev(S.rnd(N, K)), dev(S.rnd(N)), dev(S.rnd(R, N))
    y, dx, dw, db = ARENA.wide(R, N), ARENA.wide(R, K), ARENA.wide(N, K), ARENA.wide(1, N)
    p = lambda t: t.data_ptr()
    for s in [(0, N, K), (R, 0, K), (R, N, 0), (R, N, 6), (-1, N, K)]:
        refused(ops, "mtp_small_linear_fwd", p(x), p(w), p(b), p(y), *s, st())
        refused(ops, "mtp_small_linear_bwd", p(x), p(w), p(dy), p(dx), p(dw), p(db), *s, st())
    for i in range(3):
        a = [p(x), p(w), p(y)]
        a[i] = None
        refused(ops, "mtp_small_linear_fwd", a[0], a[1], p(b), a[2], R, N, K, st())
        a = [p(x), p(w), p(dy)]
        a[i] = None
        refused(ops, "mtp_small_linear_bwd", a[0], a[1], a[2], p(dx), p(dw), p(db), R, N, K, st())
    # segments: two of 4 + 4 rows
    seg = [ARENA.wide(4, K), ARENA.wide(4, K)]
    segb = [ARENA.wide(1, 4), ARENA.wide(1, 4)]
    P2, P5 = C.c_void_p * 2, C.c_void_p * 5
    I2, I5 = C.c_int64 * 2, C.c_int64 * 5
    pw, pb, rows = P2(*[p(t) for t in seg]), P2(*[p(t) for t in segb]), I2(4, 4)
    name = "mtp_small_linear_dw_segments"
    refused(ops, name, p(x), p(dy), R, N, K, 0, rows, pw, pb, st())
    refused(ops, name, p(x), p(dy), R, N, K, 5, I5(2, 2, 2, 1, 1), P5(*[p(seg[0])] * 5), P5(*[p(segb[0])] * 5), st())
    refused(ops, name, p(x), p(dy), R, N, K, 2, I2(4, 3), pw, pb, st())
    refused(ops, name, p(x), p(dy), R, N, K, 2, I2(8, 0), pw, pb, st())
    refused(ops, name, p(x), p(dy), R, N, K, 2, rows, P2(p(seg[0]), None), pb, st())
    for s in [(0, N, K), (R, 0, K), (R, N, 0), (R, N, 6)]:
        refused(ops, name, p(x), p(dy), *s, 2, rows, pw, pb, st())
    for a in [(None, p(dy), rows, pw), (p(x), None, rows, pw), (p(x), p(dy), None, pw), (p(x), p(dy), rows, None)]:
        refused(ops, name, a[0], a[1], R, N, K, 2, a[2], a[3], pb, st())
    # batched
    name = "mtp_small_linear_dw_segments_batched"
    P9, P18, P1 = C.c_void_p * 9, C.c_void_p * 18, C.c_void_p * 1
    refused(ops, name, P9(*[p(x)] * 9), P9(*[p(dy)] * 9), 9, R, N, K, 2, rows, P18(*[p(seg[0]), p(seg[1])] * 9), P18(*[p(segb[0]), p(segb[1])] * 9), st())
    refused(ops, name, P1(p(x)), P1(p(dy)), 0, R, N, K, 2, rows, pw, pb, st())
    refused(ops, name, P1(p(x)), P1(p(dy)), 1, R, N, K, 0, rows, pw, pb, st())
    refused(ops, name, P1(p(x)), P1(p(dy)), 1, R, N, K, 5, I5(2, 2, 2, 1, 1), P5(*[p(seg[0])] * 5), P5(*[p(segb[0])] * 5), st())
    refused(ops, name, P1(p(x)), P1(p(dy)), 1, R, N, K, 2, I2(4, 3), pw, pb, st())
    refused(ops, name, P1(p(x)), P1(p(dy)), 1, R, N, 0, 2, rows, pw, pb, st())
    refused(ops, name, P1(None), P1(p(dy)), 1, R, N, K, 2, rows, pw, pb, st())
    refused(ops, name, None, P1(p(dy)), 1, R, N, K, 2, rows, pw, pb, st())
    refused(ops, name, P1(p(x)), P1(p(dy)), 1, R, N, K, 2, rows, None, pb, st())
    # one row more than small_linear_dx's grid takes, with buffers of that size
    Rw = S.DX_ROWS_MAX + 1
    xr, wr, dyr = dev(S.ints(Rw, 4)), dev(S.ints(1, 4)), dev(S.ints(Rw, 1))
    dxr, dwr, dbr = ARENA.wide(Rw, 4), ARENA.wide(1, 4), ARENA.wide(1, 1)
    refused(ops, "mtp_small_linear_bwd", p(xr), p(wr), p(dyr), p(dxr), p(dwr), p(dbr), Rw, 1, 4, st())
    torch.cuda.synchronize()
    ARENA.check()
