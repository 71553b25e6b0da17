"""GPU: the LayerNorm kernels and the row reductions (csrc/layernorm.hip) where the workload runs them and the op tests did not: past one trip of their
grid-stride loops, on either side of every width at which another instantiation takes over, in the statistics regimes a one-pass variance fails, and at
the arguments they must refuse.  Every buffer comes out of the guard arena (tests/guard.py): outputs NaN-poisoned and between guards, inputs frozen, the
wrappers' partial-row workspaces poisoned and guarded; gamma, beta, layer_scale at their exact size, so a clamped column that is not clamped lands in a
guard.  Inputs, references and bounds are tests/ln_cases.py's; tests/test_ln_edges_host.py proves on the CPU what is taken for granted here.

A. Grid-trip seams: inputs whose every intermediate is exact in f32 (proved by the host test), so the kernels return the float64 result bit for bit: a
   row skipped, counted twice or added to the wrong partial row is an unequal number, not an error inside a tolerance.
B. Width seams: float64 from the dtype-rounded inputs, the existing tolerances.
C. Regimes: bound = max(the project's tolerance, 4 x the error of a float32 restatement of the kernel); kernel and restatement errors are recorded
   (conftest.record_parity, group "layernorm"; profiles/layernorm_parity_errors.json holds a run's table).
D. Refusals: the exact error text, and every output still poison.
E. Row reductions: optim_ref.exact_ints, the integer itself."""

import pytest
import torch

import guard
import ln_cases as L
import optim_ref as R
from conftest import record_parity, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
TOL = L.TOL
ARENA = None     # the running test's guard.Arena


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
    """an op INPUT: guarded and frozen"""
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t, dtype=None):
    """updated in place by contract: guarded, not frozen"""
    return ARENA.like(t, dtype=dtype or t.dtype)


def e(*shape, dtype=F32):
    """an op OUTPUT: NaN-poisoned, between guards"""
    return ARENA.empty(*shape, dtype=dtype)


def same(got, want, what):
    """got (device, f32 or bf16) holds the float64 values `want` exactly: bf16 = want rounded once"""
    g = got.cpu()
    w = want.float().to(g.dtype)          # want is an f32 number (the host test proves it): the first cast is exact
    bad = ~(g == w)                       # (NaN, a never-written element, is unequal)
    assert not bool(bad.any()), "%s: %d of %d elements differ; first at %s: got %r, want %r" % (
        what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(g[bad][0]), float(w[bad][0]))


def pair(t0=None, t1=None, n=None):
    """dgamma and dbeta adjacent in one buffer, as the flat gradient buffer holds them: one reduction launch, and what `defer` asks for"""
    buf = e(2 * n) if t0 is None else io(torch.cat([t0, t1]))
    n = n or t0.numel()
    return buf[:n], buf[n:]


# ------------------------------------------------------------------------------------------------ A: grid-trip seams, bit for bit
def _bwd_inputs(c, dtype=F32):
    return dev(c["dy"], dtype), dev(c["x"]), dev(c["mean"]), dev(c["rstd"]), dev(c["gamma"])


@pytest.mark.parametrize("rows,Cc", L.BWD_TRIP_CASES)
def test_layernorm_bwd_past_one_trip_is_exact(ops, rows, Cc):
    """plain, dgamma and dbeta in separate buffers (two reductions of a column slice each); then accumulating onto integers"""
    c = L.exact_case(rows, Cc)
    ref, _ = L.exact_bwd(c)
    dx, dg, db = e(rows, Cc), e(Cc), e(Cc)
    ops.layernorm_bwd(*_bwd_inputs(c), dx, dg, db)
    same(dx, ref["dx"], "dx"), same(dg, ref["dgamma"], "dgamma"), same(db, ref["dbeta"], "dbeta")
    ref, _ = L.exact_bwd(c, accumulate=True)
    dx, dg, db = e(rows, Cc), io(c["pre_g"]), io(c["pre_b"])
    ops.layernorm_bwd(*_bwd_inputs(c), dx, dg, db, accumulate=True)
    same(dx, ref["dx"], "dx"), same(dg, ref["dgamma"], "dgamma += "), same(db, ref["dbeta"], "dbeta +=")


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,Cc", L.BWD_TRIP_CASES)
def test_layernorm_bwd_fused_addends_and_scaled_copy_past_one_trip_are_exact(ops, rows, Cc, dtype):
    """dres, extra, and the copy scaled per sample of 7 x 293 rows: the trips after the first cross sample boundaries; a bf16 copy is the float64 value
    rounded once"""
    c = L.exact_case(rows, Cc)
    ref, _ = L.exact_bwd(c, fused=True)
    dx, dxc, (dg, db) = e(rows, Cc), e(rows, Cc, dtype=dtype), pair(n=Cc)
    ops.layernorm_bwd(*_bwd_inputs(c, dtype), dx, dg, db, dres=dev(c["dres"]), extra=dev(c["extra"]), dx_copy=dxc, copy_scale=dev(c["copy_scale"]),
                      rows_per_sample=L.RPS)
    same(dx, ref["dx"], "dx"), same(dxc, ref["dx_copy"], "dx_copy"), same(dg, ref["dgamma"], "dgamma"), same(db, ref["dbeta"], "dbeta")
    assert c["copy_scale"].numel() == -(-rows // L.RPS)


@pytest.mark.parametrize("rows,Cc", L.BWD_TRIP_CASES)
def test_layernorm_bwd_deferred_reduction_gives_the_bits_of_the_immediate_one(ops, rows, Cc):
    c = L.exact_case(rows, Cc)
    ref, _ = L.exact_bwd(c)
    jobs = []
    dx1, (dg1, db1) = e(rows, Cc), pair(n=Cc)
    ops.layernorm_bwd(*_bwd_inputs(c), dx1, dg1, db1, defer=jobs)
    assert len(jobs) == 1 and tuple(jobs[0][0].shape) == (ops.lib().mtp_layernorm_bwd_partial_rows(rows), 2 * Cc)
    dx2, (dg2, db2) = e(rows, Cc), pair(n=Cc)
    ops.layernorm_bwd(*_bwd_inputs(c), dx2, dg2, db2)
    ops.reduce_rows_deferred(jobs)
    assert not jobs
    for a, b, name in ((dx1, dx2, "dx"), (dg1, dg2, "dgamma"), (db1, db2, "dbeta")):
        same(a, ref[name], name + " (deferred)"), same(b, ref[name], name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("Cc", [4, L.C_WIDE])
@pytest.mark.parametrize("B,Hp,Wp", L.WIN_GRIDS)
def test_layernorm_bwd_window_addend_past_one_trip_is_exact(ops, B, Hp, Wp, Cc):
    """more than 2048 tokens: the row -> window arithmetic runs on a second trip"""
    c = L.exact_win_case(B, Hp, Wp, Cc)
    rows = B * Hp * Wp
    ref, _ = L.exact_bwd(c, wa=c["win_add"][c["win"]])
    dx, dg, db = e(rows, Cc), e(Cc), e(Cc)
    ops.layernorm_bwd(*_bwd_inputs(c), dx, dg, db, win_add=dev(c["win_add"]), grid=(B, Hp, Wp))
    same(dx, ref["dx"], "dx"), same(dg, ref["dgamma"], "dgamma"), same(db, ref["dbeta"], "dbeta")


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,Cc", L.BWD_TRIP_CASES)
def test_layernorm_residual_bwd_past_one_trip_is_exact(ops, rows, Cc, dtype):
    """with sample_scale; dh, dgamma, dbeta and dls, immediate (three buffers) and deferred (dgamma | dbeta adjacent)"""
    c = L.exact_case(rows, Cc)
    ref, _ = L.exact_res_bwd(c)

    def inputs():
        return (dev(c["dy"]), dev(c["x"], dtype), dev(c["mean"]), dev(c["rstd"]), dev(c["gamma"]), dev(c["beta"]), dev(c["ls"]))
    dh, dg, db, dl = e(rows, Cc, dtype=dtype), io(c["pre_g"]), io(c["pre_b"]), io(c["pre_l"])
    ops.layernorm_residual_bwd(*inputs(), dh, dg, db, dl, dev(c["sample_scale"]), L.RPS)
    same(dh, ref["dh"], "dh"), same(dg, ref["dgamma"], "dgamma"), same(db, ref["dbeta"], "dbeta"), same(dl, ref["dls"], "dls")
    jobs = []
    dh2, (dg2, db2), dl2 = e(rows, Cc, dtype=dtype), pair(c["pre_g"], c["pre_b"]), io(c["pre_l"])
    ops.layernorm_residual_bwd(*inputs(), dh2, dg2, db2, dl2, dev(c["sample_scale"]), L.RPS, defer=jobs)
    assert len(jobs) == 2
    ops.reduce_rows_deferred(jobs)
    same(dh2, ref["dh"], "dh"), same(dg2, ref["dgamma"], "dgamma (deferred)"), same(db2, ref["dbeta"], "dbeta (deferred)"), same(dl2, ref["dls"], "dls (deferred)")


@pytest.mark.parametrize("rows,Cc", L.FWD_TRIP_CASES)
def test_layernorm_forwards_past_one_trip(ops, rows, Cc):
    """every row has its own integer offset: its mean is exact and names it.  ln_fwd_kernel, then ln_res_fwd_kernel with sample_scale"""
    c = L.exact_fwd_case(rows, Cc)
    ref = c["ref"]
    y, mean, rstd = e(rows, Cc), e(rows), e(rows)
    ops.layernorm_fwd(dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), y, mean, rstd)
    for t in (y, mean, rstd):
        ARENA.check_written(t)
    same(mean, ref["mean"], "mean")
    assert rel_err(y.cpu(), ref["y"]) < TOL[F32] and rel_err(rstd.cpu(), ref["rstd"]) < TOL[F32]
    out, oact, mean2, rstd2 = e(rows, Cc), e(rows, Cc), e(rows), e(rows)
    ops.layernorm_residual_fwd(dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), dev(c["res"]), dev(c["ls"]), out, oact, mean2, rstd2, dev(c["sample_scale"]), L.RPS)
    for t in (out, oact, mean2, rstd2):
        ARENA.check_written(t)
    same(mean2, ref["mean"], "mean (residual)")
    assert rel_err(out.cpu(), ref["out"]) < TOL[F32] and rel_err(rstd2.cpu(), ref["rstd"]) < TOL[F32] and torch.equal(out, oact)


# ------------------------------------------------------------------------------------------------ B: width seams
def _seam_inputs(rows, Cc):
    return L.rnd(rows, Cc, scale=2.0) + 0.5, 1 + 0.1 * L.rnd(Cc, seed=1), 0.1 * L.rnd(Cc, seed=2)


@pytest.mark.parametrize("xdt,ydt", L.FWD_COMBOS, ids=["%s-%s" % (L.DTN[a], L.DTN[b]) for a, b in L.FWD_COMBOS])
@pytest.mark.parametrize("rows", L.SEAM_ROWS)
@pytest.mark.parametrize("Cc", L.WIDTHS)
def test_layernorm_fwd_width_seams(ops, Cc, rows, xdt, ydt):
    x, g, b = _seam_inputs(rows, Cc)
    x = L.rounded(x, xdt)
    for gelu in ([False, True] if Cc in L.GELU_WIDTHS else [False]):
        yr, mr, rr, _ = L.ln_math(x, g, b, torch.float64, gelu=gelu)
        y, mean, rstd = e(rows, Cc, dtype=ydt), e(rows), e(rows)
        ops.layernorm_fwd(dev(x, xdt), dev(g), dev(b), y, mean, rstd, gelu=gelu)
        assert rel_err(y.float().cpu(), yr) < TOL[ydt] and rel_err(mean.cpu(), mr) < 1e-5 and rel_err(rstd.cpu(), rr) < 1e-5, gelu


@pytest.mark.parametrize("dydt,xdt,dxdt", L.BWD_COMBOS, ids=["-".join(L.DTN[d] for d in c) for c in L.BWD_COMBOS])
@pytest.mark.parametrize("rows", L.SEAM_ROWS)
@pytest.mark.parametrize("Cc", L.WIDTHS)
def test_layernorm_bwd_width_seams(ops, Cc, rows, dydt, xdt, dxdt):
    """dx, its scaled copy in dy's dtype, dgamma and dbeta; mean and rstd are inputs (the float64 ones as f32)"""
    x, g, b = _seam_inputs(rows, Cc)
    x, dy = L.rounded(x, xdt), L.rnd(rows, Cc, dtype=dydt, seed=3)
    _, mr, rr, _ = L.ln_math(x, g, b, torch.float64)
    mean, rstd = mr.float(), rr.float()
    rps = 4
    cs = torch.tensor([0.5, 2.0, 1.5])[: -(-rows // rps)]
    for gelu in ([False, True] if Cc in L.GELU_WIDTHS else [False]):
        dxr, dgr, dbr = L.ln_bwd_math(dy, x, mean, rstd, g, torch.float64, b=b, gelu=gelu)
        dx, dxc, dg, db = e(rows, Cc, dtype=dxdt), e(rows, Cc, dtype=dydt), e(Cc), e(Cc)
        ops.layernorm_bwd(dev(dy, dydt), dev(x, xdt), dev(mean), dev(rstd), dev(g), dx, dg, db, beta=(dev(b) if gelu else None), gelu=gelu,
                          dx_copy=dxc, copy_scale=dev(cs), rows_per_sample=rps)
        assert rel_err(dx.float().cpu(), dxr) < (L.P_TOL if dxdt == F32 else TOL[BF16]), gelu
        assert rel_err(dxc.float().cpu(), dxr * L.per_row(cs.double(), rows, rps)[:, None]) < TOL[dydt], gelu
        assert rel_err(dg.cpu(), dgr) < L.P_TOL and rel_err(db.cpu(), dbr) < L.P_TOL, gelu


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", L.SEAM_ROWS)
@pytest.mark.parametrize("Cc", L.WIDTHS)
def test_layernorm_residual_width_seams(ops, Cc, rows, dtype):
    rps = 2
    h, g, b = _seam_inputs(rows, Cc)
    h, x, dout, ls = L.rounded(h, dtype), L.rnd(rows, Cc, seed=4), L.rnd(rows, Cc, seed=5), 0.5 * L.rnd(Cc, seed=6)
    ss = (torch.arange(-(-rows // rps)) % 3 != 1).float() / 0.8
    srow = L.per_row(ss, rows, rps)
    outr, mr, rr = L.res_fwd_math(h, g, b, x, ls, srow, torch.float64)
    out, oact, mean, rstd = e(rows, Cc), e(rows, Cc, dtype=dtype), e(rows), e(rows)
    ops.layernorm_residual_fwd(dev(h, dtype), dev(g), dev(b), dev(x), dev(ls), out, oact, mean, rstd, dev(ss), rps)
    assert rel_err(out.cpu(), outr) < TOL[F32] and rel_err(oact.float().cpu(), outr) < TOL[dtype]
    assert rel_err(mean.cpu(), mr) < 1e-5 and rel_err(rstd.cpu(), rr) < 1e-5
    dhr, dgr, dbr, dlr = L.res_bwd_math(dout, h, mean.cpu(), rstd.cpu(), g, b, ls, srow, torch.float64)
    dh, dg, db, dl = e(rows, Cc, dtype=dtype), ARENA.zeros(Cc), ARENA.zeros(Cc), ARENA.zeros(Cc)      # (the three parameter gradients accumulate)
    ops.layernorm_residual_bwd(dev(dout), dev(h, dtype), ARENA.frozen(mean), ARENA.frozen(rstd), dev(g), dev(b), dev(ls), dh, dg, db, dl, dev(ss), rps)
    assert rel_err(dh.float().cpu(), dhr) < TOL[dtype]
    assert rel_err(dg.cpu(), dgr) < L.P_TOL and rel_err(db.cpu(), dbr) < L.P_TOL and rel_err(dl.cpu(), dlr) < L.P_TOL


# ------------------------------------------------------------------------------------------------ C: statistics and GELU regimes
def _judge(tag, case, got):
    """record the kernel's and the restatement's error of every output, then hold the kernel to the bound"""
    errs = L.kernel_errors(case, got)
    late = []
    for k, err in errs.items():
        record_parity("layernorm", "%s %s kernel" % (tag, k), err)
        record_parity("layernorm", "%s %s restated" % (tag, k), case["restated"][k])
        print("%s %s: kernel %.3g restated %.3g bound %.3g" % (tag, k, err, case["restated"][k], case["bound"][k]))
        if not bool(torch.isfinite(got[k].float()).all()):
            late.append("%s: not finite" % k)
        elif not err <= case["bound"][k]:
            late.append("%s: error %.3g > bound %.3g (restated %.3g)" % (k, err, case["bound"][k], case["restated"][k]))
    assert not late, "%s: %s" % (tag, "; ".join(late))


def _run_plain(ops, case, keys):
    """the forward with and without GELU, the backward (both forms) on the kernel's own mean and rstd"""
    inp, act, Cc = case["inp"], case["act"], case["C"]
    rows = inp["x"].shape[0]
    x, g, b, dy = dev(inp["x"], act), dev(inp["gamma"]), dev(inp["beta"]), dev(inp["dy"], act)
    y, yg, mean, rstd, m2, r2 = e(rows, Cc, dtype=act), e(rows, Cc, dtype=act), e(rows), e(rows), e(rows), e(rows)
    ops.layernorm_fwd(x, g, b, y, mean, rstd)
    ops.layernorm_fwd(x, g, b, yg, m2, r2, gelu=True)
    assert torch.equal(mean, m2) and torch.equal(rstd, r2)
    ARENA.frozen(mean, rstd)
    got = dict(y=y, y_gelu=yg, mean=mean, rstd=rstd)
    for sfx, gelu in (("", False), ("_gelu", True)):
        dx, dg, db = e(rows, Cc, dtype=act), e(Cc), e(Cc)
        ops.layernorm_bwd(dy, x, mean, rstd, g, dx, dg, db, beta=(b if gelu else None), gelu=gelu)
        got.update({"dx" + sfx: dx, "dgamma" + sfx: dg, "dbeta" + sfx: db})
    return {k: v.cpu() for k, v in got.items() if k in keys}


@pytest.mark.parametrize("act", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", L.REGIME_WIDTHS)
@pytest.mark.parametrize("regime", L.REGIMES)
def test_layernorm_statistics_regimes(ops, regime, Cc, act):
    """rows far from zero, with one huge channel, with a variance near, far below and at zero against eps: a variance taken as E[x^2] - mean^2 misses these
    bounds tenfold in offset_1e3, offset_neg_small_std and near_eps (test_ln_edges_host.py)"""
    case = L.regime_case(regime, Cc, act)
    got = _run_plain(ops, case, ("y", "y_gelu", "mean", "rstd", "dx", "dgamma", "dbeta"))
    if regime == "constant" and act == F32:
        assert torch.equal(got["y"], case["inp"]["beta"].expand(L.REGIME_ROWS, Cc)), "a constant row must give y == beta exactly"
        assert bool(torch.isfinite(got["dx"]).all())
    _judge("%s C%d %s" % (regime, Cc, L.DTN[act]), case, got)


@pytest.mark.parametrize("act", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", L.REGIME_WIDTHS)
@pytest.mark.parametrize("regime", L.REGIMES)
def test_layernorm_residual_statistics_regimes(ops, regime, Cc, act):
    case = L.regime_case(regime, Cc, act)
    inp = case["inp"]
    rows = inp["x"].shape[0]
    h, g, b, ls, ss = dev(inp["x"], act), dev(inp["gamma"]), dev(inp["beta"]), dev(inp["ls"]), dev(inp["sample_scale"])
    out, oact, mean, rstd = e(rows, Cc), e(rows, Cc, dtype=act), e(rows), e(rows)
    ops.layernorm_residual_fwd(h, g, b, dev(inp["res"]), ls, out, oact, mean, rstd, ss, inp["rps"])
    ARENA.frozen(mean, rstd)
    dh, dg, db, dl = e(rows, Cc, dtype=act), ARENA.zeros(Cc), ARENA.zeros(Cc), ARENA.zeros(Cc)
    ops.layernorm_residual_bwd(dev(inp["dout"]), h, mean, rstd, g, b, ls, dh, dg, db, dl, ss, inp["rps"])
    got = dict(out=out, out_act=oact, res_mean=mean, res_rstd=rstd, dh=dh, res_dgamma=dg, res_dbeta=db, dls=dl)
    _judge("%s C%d %s" % (regime, Cc, L.DTN[act]), case, {k: v.cpu() for k, v in got.items()})


@pytest.mark.parametrize("act", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", L.REGIME_WIDTHS)
def test_layernorm_fused_gelu_over_its_whole_range(ops, Cc, act):
    """z = xhat gamma + beta over [-12, 12] and exactly 0: gelu and gelu' outside |z| < 4, against the float64 erf form"""
    case = L.gelu_case(Cc, act)
    _judge("gelu_spread C%d %s" % (Cc, L.DTN[act]), case, _run_plain(ops, case, ("y_gelu", "dx_gelu", "dgamma_gelu", "dbeta_gelu")))


# ------------------------------------------------------------------------------------------------ D: refusals, nothing launched
@pytest.mark.parametrize("entry,over,text", L.REFUSALS, ids=[L.refusal_id(r) for r in L.REFUSALS])
def test_refused_calls_raise_and_write_nothing(ops, entry, over, text):
    """real, tiny buffers: every input frozen, every output a poisoned buffer none of which may change"""
    src = dev(torch.zeros(64))

    def ptr(name, kind, i):
        return src.data_ptr() if kind == "in" else ARENA.wide(1, 64).data_ptr()           # no column registered: all of it must stay poison
    want = L.first_check(entry, over)[2]
    with pytest.raises(RuntimeError, match=L.ERR_TEXT[want] % entry):
        ops.check(L.refused_call(ops.lib(), entry, over, ptr, torch.cuda.current_stream().cuda_stream), entry)
    torch.cuda.synchronize()
    ARENA.check()


# ------------------------------------------------------------------------------------------------ E: row reductions, the integer itself
def _base(cols):
    return (torch.arange(cols) % 11 - 5).float()


@pytest.mark.parametrize("cols", L.RED_COLS)
@pytest.mark.parametrize("rows", L.RED_ROWS)
def test_reduce_rows_returns_the_integers(ops, rows, cols):
    """mtp_reduce_rows_f32 over a whole buffer and over a column slice of it (ld = cols + 8), into poison and on top of integers; the batched launcher
    (ops.reduce_rows_deferred) with one buffer and with two"""
    ld = cols + L.RED_PAD
    x, x2 = R.exact_ints(rows * ld, seed=6).view(rows, ld), R.exact_ints(rows * ld, seed=7).view(rows, ld)
    d1, d2 = dev(x), dev(x2)
    p1, p2 = d1[:, 4:4 + cols], d2[:, 4:4 + cols]
    w1, w2 = x[:, 4:4 + cols].double().sum(0), x2[:, 4:4 + cols].double().sum(0)
    same(ops.reduce_rows(d1, e(ld)), x.double().sum(0), "whole")
    same(ops.reduce_rows(p1, e(cols)), w1, "slice")
    acc = ops.reduce_rows(p1, io(_base(cols)), accumulate=True)
    same(acc, _base(cols).double() + w1, "slice +=")
    same(ops.reduce_rows(p2, acc, accumulate=True), _base(cols).double() + w1 + w2, "slice += +=")
    o1, o2, o3 = e(cols), io(_base(cols)), io(_base(cols))
    ops.reduce_rows_deferred([(p1, o1, False)])
    ops.reduce_rows_deferred([(p1, o2, True), (p2, o3, True)])
    same(o1, w1, "batched, one"), same(o2, _base(cols).double() + w1, "batched, first of two"), same(o3, _base(cols).double() + w2, "batched, second of two")


@pytest.mark.parametrize("n,rows,cols", L.RED_BATCHES)
def test_reduce_rows_batches_return_the_integers(ops, n, rows, cols):
    """1, 2, 32 and 33 equally shaped column slices in one list: at most 32 per launch, so 33 is two launches"""
    ld = cols + L.RED_PAD
    x = R.exact_ints(n * rows * ld, seed=8).view(n, rows, ld)
    want = x[:, :, :cols].double().sum(1)
    d = dev(x)
    out = e(n, cols)
    jobs = [(d[i][:, :cols], out[i], False) for i in range(n)]
    ops.reduce_rows_deferred(jobs)
    assert not jobs
    same(out, want, "into poison")
    acc = io(_base(cols).repeat(n, 1))
    ops.reduce_rows_deferred([(d[i][:, :cols], acc[i], True) for i in range(n)])
    same(acc, _base(cols).double() + want, "on top of integers")


def test_reduce_rows_one_list_mixing_two_shapes(ops):
    """two shapes interleaved in one list: one launch per shape, every buffer to its own output"""
    shapes = [(17, 257), (33, 4100), (17, 257), (33, 4100), (17, 257)]
    xs = [R.exact_ints(r * (c + L.RED_PAD), seed=9 + i).view(r, c + L.RED_PAD) for i, (r, c) in enumerate(shapes)]
    outs = [e(c) for _, c in shapes]
    ops.reduce_rows_deferred([(dev(x)[:, :c], o, False) for x, o, (_, c) in zip(xs, outs, shapes)])
    for i, (x, o, (_, c)) in enumerate(zip(xs, outs, shapes)):
        same(o, x[:, :c].double().sum(0), "buffer %d" % i)
