"""CPU: what tests/test_hip_ln_edges.py takes for granted about its own inputs and bounds, asserted on the very inputs of the GPU tests (tests/ln_cases.py):
the exact inputs ARE exact (every intermediate a multiple of 2^-k whose absolute values, times 2^k, sum to less than 2^24); the row counts give the trips
and workgroup counts they are named for under the library's own mtp_layernorm_bwd_partial_rows; every width runs on the instantiation on the intended
side of its seam; the float32 restatement the regime bounds are derived from is the kernels' arithmetic, and a one-pass variance misses those bounds by
10 x where the regime is there to catch it; every refused call is refused by the check it is named after, which is where the table says it is."""
import os

import pytest
import torch
import torch.nn.functional as F

import ln_cases as L
import optim_ref as R
from oracle import vit_rvsa_oracle as O

F32, BF16, F64 = L.F32, L.BF16, L.F64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mtp_amd", "csrc")


def lib():
    from mtp_amd import _lib
    return _lib.load()


def assert_exact(what, terms):
    for t in terms:
        k, worst = L.exactness(t)
        assert k is not None, "%s: %s is no multiple of a power of two" % (what, t[0])
        assert worst < 2 ** 24, "%s: %s: sum of |terms| x 2^%d = %g >= 2^24" % (what, t[0], k, worst)


def f32_exact(t):
    return torch.equal(t.float().double(), t)


# ------------------------------------------------------------------------------------------------ A: exact inputs
@pytest.mark.parametrize("rows,C", L.BWD_TRIP_CASES)
def test_backward_trip_inputs_are_exact_in_f32_in_any_order(rows, C):
    c = L.exact_case(rows, C)
    for kw in (dict(), dict(fused=True), dict(accumulate=True)):
        res, terms = L.exact_bwd(c, **kw)
        assert_exact("ln_bwd %s" % kw, terms)
        assert all(f32_exact(v) for v in res.values())
    res, terms = L.exact_res_bwd(c)
    assert_exact("ln_res_bwd", terms)
    assert all(f32_exact(v) for v in res.values())
    # the inputs are what the recipe says, in earnest: every value of every set is there, and the result is no row of zeros
    assert set(c["mean"].unique().tolist()) == {-1.0, 0.0, 1.0} and set(c["rstd"].unique().tolist()) == {0.5, 1.0, 2.0}
    assert set(c["x"].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(c["dy"].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert c["ns"] == -(-rows // L.RPS) >= 1 and (4 * 512) % L.RPS != 0
    assert float(res["dgamma"].abs().max()) > 0 and float(res["dls"].abs().max()) > 0 and float(res["dh"].abs().max()) > 0


@pytest.mark.parametrize("B,Hp,Wp", L.WIN_GRIDS)
@pytest.mark.parametrize("C", [4, L.C_WIDE])
def test_window_addend_inputs_are_exact_and_past_one_trip(B, Hp, Wp, C):
    c = L.exact_win_case(B, Hp, Wp, C)
    assert B * Hp * Wp > 4 * L.bwd_grid(B * Hp * Wp) and L.trips(B * Hp * Wp, L.bwd_grid(B * Hp * Wp)) == 2
    res, terms = L.exact_bwd(c, wa=c["win_add"][c["win"]])
    assert_exact("ln_bwd win", terms)
    assert sorted(set(c["win"].tolist())) == list(range(c["win_add"].shape[0]))          # every window holds a token


def test_the_exactness_proof_refuses_what_is_not_exact():
    third = torch.full((4, 4), 1.0 / 3.0, dtype=F64)
    assert L.exactness(("third", [third], None))[0] is None
    big = torch.full((2 ** 12, 1), 2.0 ** 12 + 0.5, dtype=F64)
    k, worst = L.exactness(("big", [big], 0))
    assert k == 1 and worst >= 2 ** 24 and L.exactness(("big", [big], None))[1] < 2 ** 24
    with pytest.raises(AssertionError):
        assert_exact("x", [("big", [big], 0)])


@pytest.mark.parametrize("rows,C", L.FWD_TRIP_CASES)
def test_forward_trip_inputs_have_an_exact_mean_that_names_the_row(rows, C):
    c = L.exact_fwd_case(rows, C)
    x = c["x"].double()
    assert_exact("ln_fwd", [("row sum", [x], 1), ("mean", [x.sum(1) / C], None)])
    mean = c["ref"]["mean"]
    assert f32_exact(mean) and torch.equal(mean, x.sum(1) / C)
    step = L.LN_ROWS_PER_WG * L.ln_grid(rows)
    # a row and the row one trip later (the same wave of the same workgroup) differ in their mean by more than the sum of the random part can undo
    assert bool(((mean[step:] - mean[:-step]).abs() > 4).all()) if rows > step else True
    assert bool(((mean[1:] - mean[:-1]).abs() > 0).float().mean() > 0.9)


# ------------------------------------------------------------------------------------------------ A: the launch rule
def test_row_counts_give_the_trips_and_workgroups_they_are_named_for():
    rows_of = lib().mtp_layernorm_bwd_partial_rows
    got = [(r, rows_of(r), L.trips(r, rows_of(r))) for r in L.BWD_ROWS]
    assert got == [(2048, 512, 1), (2049, 512, 2), (4097, 512, 3), (65536, 512, 32), (65537, 1024, 17), (262144, 1024, 64), (262145, 2048, 33)]
    for r in list(range(1, 4200)) + [65535, 65536, 65537, 262143, 262144, 262145, 262146, 524288, 2 ** 31 - 1]:
        assert rows_of(r) == L.bwd_grid(r), r
    assert [(r, L.ln_grid(r), L.trips(r, L.ln_grid(r))) for r in L.FWD_ROWS] == [(8192, 2048, 1), (8193, 2048, 2), (16385, 2048, 3)]
    assert {C for _, C in L.BWD_TRIP_CASES} == {4, 512} == {C for _, C in L.FWD_TRIP_CASES}
    assert max(r for r, C in L.BWD_TRIP_CASES if C == 512) == 4097 and [r for r, C in L.FWD_TRIP_CASES if C == 512] == [8193]
    assert max(r * C for r, C in L.BWD_TRIP_CASES + L.FWD_TRIP_CASES) * 4 <= 17 << 20           # the largest buffer of the trip cases


@pytest.mark.parametrize("what,line,text", L.RESTATES, ids=["%s:%d" % (r[0], r[1]) for r in L.RESTATES])
def test_restated_lines_are_where_they_are_said_to_be(what, line, text):
    with open(os.path.join(CSRC, "layernorm.hip")) as f:
        got = f.read().split("\n")[line - 1]
    assert text in got, "layernorm.hip:%d no longer holds what %s restates: %r" % (line, what, got.strip())


def test_the_python_side_cuts_batches_where_the_table_says():
    from mtp_amd import ops
    assert ops.REDUCE_BATCH_MAX == L.REDUCE_BATCH_MAX == 32


# ------------------------------------------------------------------------------------------------ B: widths
def test_every_width_runs_on_the_intended_side_of_its_seam():
    assert [L.mv_of(C) for C in L.WIDTHS] == [1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 8, 8]
    assert [L.masked_lanes(C) for C in L.WIDTHS] == [1, 0, 63, 0, 63, 0, 63, 0, 127, 0, 127, 1, 0]
    assert {L.mv_of(C) for C in L.WIDTHS} == set(L.LN_MVS) == {L.mv_of(C) for C in range(4, 2049, 4)}
    for C in range(4, 2049, 4):
        assert 64 * L.mv_of(C) * 4 >= C                                          # the instantiation holds the row
    assert set(L.GELU_WIDTHS) <= set(L.WIDTHS) and len(L.GELU_WIDTHS) == 4 and {L.masked_lanes(C) > 0 for C in L.GELU_WIDTHS} == {True, False}
    assert [L.mv_of(C) for C in L.REGIME_WIDTHS] == [1, 2, 4, 8]
    for rows in L.SEAM_ROWS:          # one live wave in the last workgroup
        assert rows % 4 == 1 and L.ln_grid(rows) == L.bwd_grid(rows) == rows // 4 + 1
    assert len(set(L.FWD_COMBOS)) == 4 and set(L.BWD_COMBOS) == {tuple({0: F32, 1: BF16}[d] for d in c) for c in L.SUPPORTED_BWD}


# ------------------------------------------------------------------------------------------------ C: the one statement of the arithmetic
def test_the_float64_statement_is_the_oracles_and_autograds():
    rows, C = 9, 260
    x, g, b, dy = L.rnd(rows, C, scale=2.0) + 0.5, 1 + 0.1 * L.rnd(C, seed=1), 0.1 * L.rnd(C, seed=2), L.rnd(rows, C, seed=3)
    y, mu, rs, z = L.ln_math(x, g, b, F64)
    yo, mo, ro = O.layernorm_fwd(x.double(), g.double(), b.double())
    assert torch.equal(y, yo) and torch.equal(mu, mo) and torch.equal(rs, ro) and torch.equal(y, z)
    assert L.rel_err(y, F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-6)) < 1e-14
    assert L.rel_err(L.ln_math(x, g, b, F64, gelu=True)[0], O.gelu(yo)) < 1e-15 and L.rel_err(L.dgelu_math(yo), O.dgelu(yo)) < 1e-15
    for got, want in zip(L.ln_bwd_math(dy, x, mu, rs, g, F64), O.layernorm_bwd(dy.double(), x.double(), mo, ro, g.double())):
        assert L.rel_err(got, want) < 1e-14
    # with GELU: autograd through gelu(layer_norm)
    xr, gr, br = (t.double().clone().requires_grad_(True) for t in (x, g, b))
    F.gelu(F.layer_norm(xr, (C,), gr, br, 1e-6)).backward(dy.double())
    for got, want in zip(L.ln_bwd_math(dy, x, mu, rs, g, F64, b=b, gelu=True), (xr.grad, gr.grad, br.grad)):
        assert L.rel_err(got, want) < 1e-12
    # the residual pair
    res, ls, dout = L.rnd(rows, C, seed=4), 0.5 * L.rnd(C, seed=5), L.rnd(rows, C, seed=6)
    srow = L.per_row(torch.tensor([1.25, 0.0, 0.5, 1.25, 1.25]), rows, 2)
    hr, gr, br, lr = (t.double().clone().requires_grad_(True) for t in (x, g, b, ls))
    ref = res.double() + srow.double()[:, None] * lr * F.layer_norm(hr, (C,), gr, br, 1e-6)
    ref.backward(dout.double())
    out, rmu, rrs = L.res_fwd_math(x, g, b, res, ls, srow, F64)
    assert L.rel_err(out, ref.detach()) < 1e-14
    for got, want in zip(L.res_bwd_math(dout, x, rmu, rrs, g, b, ls, srow, F64), (hr.grad, gr.grad, br.grad, lr.grad)):
        assert L.rel_err(got, want) < 1e-12
    # the exact references of section A are this statement too
    c = L.exact_case(9, 8)
    ea, _ = L.exact_bwd(c)
    for got, want in zip(L.ln_bwd_math(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], F64), (ea["dx"], ea["dgamma"], ea["dbeta"])):
        assert torch.equal(got, want)
    er, _ = L.exact_res_bwd(c)
    srow = L.per_row(c["sample_scale"], 9)
    for got, want, pre in zip(L.res_bwd_math(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["ls"], srow, F64),
                              (er["dh"], er["dgamma"], er["dbeta"], er["dls"]), (0, c["pre_g"], c["pre_b"], c["pre_l"])):
        assert torch.equal(got + pre, want)


@pytest.mark.parametrize("act", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", L.REGIME_WIDTHS)
@pytest.mark.parametrize("regime", L.REGIMES)
def test_the_restatement_stays_inside_its_own_bound(regime, C, act):
    case = L.regime_case(regime, C, act)
    fl = L.floors(act)
    assert set(case["bound"]) == set(fl) == set(case["ref"])
    for k, b in case["bound"].items():
        assert case["restated"][k] <= b / L.MARGIN or b == fl[k], (k, case["restated"][k], b)
        assert fl[k] <= b < 0.05 and all(bool(torch.isfinite(t).all()) for t in (case["ref"][k],)), (k, b)
    x = case["inp"]["x"]
    assert torch.equal(x, L.rounded(x, act))                                      # the inputs are what the dtype holds
    if regime == "constant":
        assert (case["restated"]["y"] == 0.0 or act == BF16) and torch.equal(case["ref"]["y"], case["inp"]["beta"].double().expand(L.REGIME_ROWS, C))
        assert L.rel_err(case["ref"]["rstd"], torch.full((L.REGIME_ROWS,), 1000.0)) < 1e-12
        assert set(x[:, 0].tolist()) == set(L.CONSTANTS)


def test_the_regimes_are_what_their_names_say():
    for C in L.REGIME_WIDTHS:
        ref = {r: L.regime_case(r, C, F32)["ref"] for r in L.REGIMES}
        var = {r: 1.0 / ref[r]["rstd"] ** 2 - L.EPS for r in L.REGIMES}
        assert float(var["near_eps"].min()) > 0.02 * L.EPS and float(var["near_eps"].max()) < 5 * L.EPS
        assert float(var["tiny"].max()) < 0.05 * L.EPS and float(var["big"].min()) > 1e6 and float(var["constant"].abs().max()) < 1e-12
        assert float((ref["offset_1e3"]["mean"] - 1000).abs().max()) < 3 and float((ref["offset_neg_small_std"]["mean"] + 300).abs().max()) < 0.2
        x = L.regime_case("spike", C, F32)["inp"]["x"]
        assert bool(((x == 3000.0).sum(1) == 1).all())
    # the bounds the issue's measurements lead one to expect (4 x its two-pass figures); offset_neg_small_std is the one above TOL: its mean is an f32 near 300
    for C in L.REGIME_WIDTHS:
        assert L.regime_case("offset_1e3", C, F32)["bound"]["y"] < 1e-3 and L.regime_case("near_eps", C, F32)["bound"]["y"] < 1e-3
        assert L.regime_case("offset_neg_small_std", C, F32)["bound"]["y"] < 1e-2


@pytest.mark.parametrize("C", L.REGIME_WIDTHS)
@pytest.mark.parametrize("regime", L.ONE_PASS_MUST_MISS)
def test_a_one_pass_variance_misses_the_bound_tenfold(regime, C):
    """the condition the regime exists for: the same restatement with var = E[x^2] - mean^2 is at least 10 x outside the bound of y, of rstd and of the
    residual output -- a kernel that dropped the centred second pass cannot pass"""
    case = L.regime_case(regime, C, F32)
    bad = L.evaluate(case["inp"], F32, F32, one_pass=True)
    for k in ("y", "rstd", "out"):
        err = L.rel_err(bad[k], case["ref"][k])
        assert err >= L.ONE_PASS_FACTOR * case["bound"][k], (k, err, case["bound"][k])


@pytest.mark.parametrize("act", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", L.REGIME_WIDTHS)
def test_the_gelu_case_spreads_z_over_its_whole_range(C, act):
    case = L.gelu_case(C, act)
    inp = case["inp"]
    z = L.ln_math(inp["x"], inp["gamma"], inp["beta"], F64)[3]
    assert bool((z[:, 0] == 0).all()) and float(z.min()) < (-8 if C > 4 else -4) and float(z.max()) > (8 if C > 4 else 4) and float(z.abs().max()) < 20
    assert int((z.abs() > 4).sum()) > 0.05 * z.numel() and int((z.abs() < 1).sum()) > 0.05 * z.numel()
    for k in ("y_gelu", "dx_gelu", "dgamma_gelu", "dbeta_gelu"):
        assert bool(torch.isfinite(case["ref"][k]).all()) and case["restated"][k] <= case["bound"][k] < 0.05


# ------------------------------------------------------------------------------------------------ D: refusals
@pytest.mark.parametrize("entry,over,text", L.REFUSALS, ids=[L.refusal_id(r) for r in L.REFUSALS])
def test_every_refusal_is_refused_by_the_check_it_names(entry, over, text):
    """the restated checks, walked in source order, stop at the named one -- so the call passed every check before it -- that check is where the table says,
    and the library itself gives its return value (the argument checks dereference nothing: P is never read)"""
    hit = L.first_check(entry, over)
    assert hit is not None and hit[0] == text, (hit, text)
    with open(os.path.join(CSRC, "layernorm.hip")) as f:
        src = f.read().split("\n")
    assert text in src[hit[1] - 1], "layernorm.hip:%d: %r" % (hit[1], src[hit[1] - 1].strip())
    start = max(i for i in range(hit[1]) if src[i].startswith('extern "C"'))
    assert (entry + "(") in src[start], "layernorm.hip:%d is not inside %s" % (hit[1], entry)
    P = 1 << 20
    assert L.refused_call(lib(), entry, over, lambda name, kind, i: P) == hit[2]
    assert L.first_check(entry, {}) is None                                      # ... and nothing refuses the call it was derived from


def test_the_refusal_table_covers_what_it_must():
    by = {}
    for entry, over, text in L.REFUSALS:
        by.setdefault(entry, []).append((over, text))
    ln = [e for e in L.ENTRIES if "layernorm" in e]
    for e in ln:
        assert {o["C"] for o, _ in by[e] if "C" in o} >= {0, -4, 6, 2052} and any(o.get("rows") == 0 for o, _ in by[e])
    for e in ln[1:]:
        assert any(o.get("rows", 0) > L.INT32_MAX for o, _ in by[e])
    # C = 0 and C = -4 reach the kernels' `gamma + 4 * (nv - 1)` unless this very check stops them: nothing before it does
    for e in ("mtp_layernorm_bwd", "mtp_layernorm_bwd_win"):
        for Cc in (0, -4):
            others = [c for c in L.CHECKS[e] if c[0] != "C <= 0"]
            assert not any(pred(L.resolve(e, dict(C=Cc))) for _, _, _, pred in others)
    assert set(by) == set(L.ENTRIES)
    for e, checks in L.CHECKS.items():          # every restated check but the null-pointer lists of the reductions' siblings is the reason of some case
        named = {t for _, t in by[e]}
        assert {c[0] for c in checks if not c[0].startswith("!")} - named <= {"R <= 0", "C <= 0", "rows > INT32_MAX"}, e


# ------------------------------------------------------------------------------------------------ E: reductions
def test_reduction_inputs_are_exact_and_the_sizes_sit_on_their_seams():
    for rows in L.RED_ROWS:
        for cols in L.RED_COLS:
            n = rows * (cols + L.RED_PAD)
            assert n < 2 ** 24 and rows + 5 < 2 ** 24          # exact_ints: values in {-1, 0, 1}; any partial column sum, with a preset of |v| <= 5, is an integer <= rows + 5
    x = R.exact_ints(2049 * 4108, seed=5).view(2049, 4108)
    assert set(x.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert_exact("column sums", [("sum", [x.double()], 0)])
    # column_sum: every remainder after the passes of 8 and of 4, from the plain launcher's pieces
    pieces = set()
    for rows in L.RED_ROWS:
        for cols in L.RED_COLS:
            s, rpb = L.plain_splits(rows, cols)
            pieces |= {rpb, rows - (s - 1) * rpb}
            for n in (1, 2):
                s, rpb = L.batched_splits(rows, cols, n)
                pieces |= {rpb, rows - (s - 1) * rpb}
                assert (s - 1) * rpb < rows <= s * rpb
    assert {L.column_sum_passes(p)[1:] for p in pieces} >= {(a, b) for a in (0, 1) for b in (0, 1, 2, 3)}
    assert any(L.column_sum_passes(p)[0] > 1 for p in pieces)
    # the batched rows / 16 rule on both sides, and past its first step
    assert [L.batched_splits(r, 1, 1)[0] for r in (15, 16, 17, 31, 33, 512, 513)] == [1, 1, 1, 1, 2, 32, 31]
    assert [L.batched_splits(r, 1, 1)[1] for r in (15, 16, 31, 33)] == [15, 16, 31, 17]
    # 4100 columns: 17 column blocks; 1024 / 17 = 60 pieces of 35 rows -> 59, 2048 / 17 = 120 of 18 -> 114: no powers of two, a short last piece
    assert L.plain_splits(2049, 4100) == (59, 35) and L.batched_splits(2049, 4100, 1) == (114, 18) and L.batched_splits(2049, 4100, 2) == (59, 35)
    assert [L.plain_splits(2049, c) for c in (1, 255, 256, 257)] == [(683, 3)] * 3 + [(410, 5)]
    # the batch table: 33 = two launches (32 + 1); every n at every shape; the shapes straddle rows / 16 and 2048 / (col_blocks n)
    assert {n for n, _, _ in L.RED_BATCHES} == {1, 2, 32, 33} and L.REDUCE_BATCH_MAX == 32
    assert L.batched_splits(33, 4100, 32) == (2, 17) and L.batched_splits(33, 4100, 1) == (2, 17) and L.batched_splits(513, 255, 32) == (31, 17)
    assert L.batched_splits(513, 255, 1) == (31, 17) and L.batched_splits(17, 257, 32)[0] == 1
