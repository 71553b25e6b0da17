"""CPU: what tests/test_hip_decode_edges.py takes for granted about its own inputs and bounds, asserted on the very inputs of the GPU tests
(tests/decode_cases.py): the section A inputs ARE exact (the absolute values of the terms of every sum of the statistics kernels add up to less than
2^24); the row counts give the chunk lengths, ragged chunks and empty chunks they are named for under the library's own mtp_bn_partial_rows; lin_range
covers every output that lin_index gives a non-zero weight, with the slack it has left; the float32 restatement the regime bounds come from is the
kernels' arithmetic and stays inside them, and a one-pass variance misses them tenfold where the regime exists to catch it; every refused call is
refused by the check it is named after."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_cases as D

F32, BF16, F64 = D.F32, D.BF16, D.F64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mtp_amd", "csrc")


def lib():
    from mtp_amd import _lib
    return _lib.load()


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ A: exact inputs, chunk arithmetic
@pytest.mark.parametrize("C", D.BN_CHANNELS)
@pytest.mark.parametrize("rows", D.BN_ROWS)
def test_section_a_inputs_are_exact_in_f32_in_any_order(rows, C):
    c = D.exact_bn_case(rows, C)
    for name, t in D.exact_bn_terms(c):
        assert torch.equal(t, t.round()), name                                   # integers
        assert float(t.abs().sum(0).max()) < 2 ** 24, name                       # ... whose absolute values sum to less than 2^24: any partial sum is an f32 number
    for center in (False, True):
        for relu in (False, True):
            for s in D.exact_bn_sums(c, center, relu):
                assert torch.equal(s.float().double(), s) and float(s.abs().max()) > 0
    for k in ("x", "dy", "center"):                                              # bf16 numbers, all of them, and every value of the recipe occurs
        assert torch.equal(c[k].to(BF16).float(), c[k])
    assert set(c["x"].unique().tolist()) | set(c["dy"].unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    if rows < 64:
        return
    assert set(c["x"].unique().tolist()) == set(c["dy"].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    # the backward's identity statistics make xhat = x and the mask x > 0 in f32 exactly
    xh = (c["x"] - c["mean"]) * c["rstd"]
    assert torch.equal(xh, c["x"]) and torch.equal(xh * c["gamma"] + c["beta"] > 0, c["x"] > 0)
    # neighbouring rows differ (a row taken twice for its neighbour is another sum) -- over all channels together, for the four channels
    assert float((c["x"][1:] != c["x"][:-1]).any(1).float().mean()) > 0.99


def test_row_counts_give_the_chunks_they_are_named_for():
    rows_of = lib().mtp_bn_partial_rows
    for r in list(range(1, 4200)) + [32767, 32768, 32769, 33281, 65536, 2 ** 31 - 1, 2 ** 40]:
        assert rows_of(r) == D.partial_rows(r), r
    assert rows_of(0) < 0 and rows_of(-5) < 0
    assert D.BN_ROWS == sorted(D.BN_CHUNKING)
    for r in D.BN_ROWS:
        nb, chunk, ragged, rest, empty = got = D.chunking(r, rows_of(r))
        assert got == D.BN_CHUNKING[r], (r, got)
        # the chunks, walked as the kernel walks them: r0 = b * chunk, r1 = min(rows, r0 + chunk)
        lens = [max(0, min(r, (b + 1) * chunk) - b * chunk) for b in range(nb)]
        assert sum(lens) == r and lens.count(0) == empty and [b for b, n in enumerate(lens) if 0 < n < chunk] == ([ragged] if ragged is not None else [])
        assert ragged is None or lens[ragged] == rest
    # what the issue names them for: a chunk shorter than the four waves; one whose waves take 2, 1, 1, 1 rows; a ragged last chunk of the 64-row rule;
    # the last exact division; chunks of 65 and 66 rows (wave 0 takes 17 rows, wave 3 takes 16) with a ragged chunk and seven empty workgroups behind it
    assert D.chunking(3)[1] < D.BN_WAVES < D.chunking(5)[1] and D.chunking(32769)[1:] == (65, 504, 9, 7) and D.chunking(33281)[1] == 66
    assert 512 * 65 > 32769 and D.chunking(2400)[:4] == (38, 64, 37, 32) and 2400 == 6 * 20 * 20
    assert 0 < D.chunking(32769)[3] < 3 * D.BN_WAVES and D.chunking(32769)[3] % D.BN_WAVES != 0       # the ragged chunk's waves take 3, 2, 2, 2 rows
    assert max(r * (C + 2 * D.SLICE_PAD) * 4 for r in D.BN_ROWS for C in D.BN_CHANNELS) < 40 << 20    # the largest buffer
    src = source("decode_head.hip")
    assert "const int64_t nb = bn_partial_rows(rows), chunk = (rows + nb - 1) / nb;" in src
    assert "int64_t nb = (rows + 63) / 64;" in src and "return nb < 512 ? nb : 512;" in src
    assert "for (int64_t r = r0 + wv; r < r1; r += 4)" in src and "r1 = min(rows, r0 + chunk)" in src
    assert (D.BN_CHANNELS[1] // 4 + 63) // 64 == 2 and D.BN_CHANNELS[1] // 4 - 64 == 1               # C = 260: one live lane in the second channel workgroup


@pytest.mark.parametrize("C", D.BN_CHANNELS)
@pytest.mark.parametrize("rows", [3, 5])
def test_small_rows_bound_holds_for_a_float32_evaluation(rows, C):
    """bn_dx_small_rows_bound is tests/test_hip_edges.py's, at the row counts of this sweep: a float32 evaluation of the float64 reference stays inside a
    tenth of it on the very inputs of the GPU test"""
    import test_hip_edges as E
    c = D.bn_random_case(rows, C)
    assert D.bn_dx_small_rows_bound(c["x"], c["gamma"], c["dy"]) == E.bn_dx_small_rows_bound(c["x"], c["gamma"], c["dy"]) > 0
    dx32 = D.bn_autograd(c["x"], c["gamma"], c["beta"], c["dy"], dtype=F32)[2]
    far = (c["pre"].abs() > 1e-5).double()
    err = float(((dx32.double() - c["dx"]) * far).abs().max())
    assert err < 0.1 * D.bn_dx_small_rows_bound(c["x"], c["gamma"], c["dy"]), err
    assert rows < D.SMALL_ROWS <= min(r for r in D.BN_ROWS if r > 5)


# ------------------------------------------------------------------------------------------------ B: regimes
def test_the_float64_statement_is_torchs_batch_norm():
    g = torch.Generator().manual_seed(3)
    rows, C = 37, 8
    inp = dict(x=2 + torch.randn(rows, C, generator=g), gamma=1 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
               dy=torch.randn(rows, C, generator=g), rmean=torch.randn(C, generator=g), rvar=0.5 + torch.rand(C, generator=g))
    for relu in (True, False):
        ref = D.bn_math(inp, F64, relu=relu)
        xr, gr, br = (inp[k].double().clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
        rm, rv = inp["rmean"].double().clone(), inp["rvar"].double().clone()
        y = F.batch_norm(xr, rm, rv, gr, br, True, D.BN_MOMENTUM, float(np.float32(D.BN_EPS)))
        y = F.relu(y) if relu else y
        y.backward(inp["dy"].double())
        for k, want in dict(y=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad, rmean=rm, rvar=rv, mean=inp["x"].double().mean(0)).items():
            assert D.rel_err(ref[k], want) < 1e-7, k                           # (momentum is the f32 0.1 in the kernel and here)
        pre, y2, dx, dg, db = D.bn_autograd(inp["x"], inp["gamma"], inp["beta"], inp["dy"], relu=relu)
        assert D.rel_err(ref["y"], y2) < 1e-9 and D.rel_err(ref["dx"], dx) < 1e-9 and D.rel_err(ref["dgamma"], dg) < 1e-9


@pytest.mark.parametrize("name,rows", D.REGIMES)
def test_the_restatement_stays_inside_the_bound_it_produces(name, rows):
    case = D.regime_case(name, rows)
    ref, inp = case["ref"], case["inp"]
    assert set(case["bound"]) == set(D.FLOORS) == set(ref)
    for k, b in case["bound"].items():
        assert case["restated"][k] <= b / D.MARGIN or b == D.FLOORS[k], (k, case["restated"][k], b)
        assert D.FLOORS[k] <= b < 5e-3 and bool(torch.isfinite(ref[k]).all()), (k, b)
    # no pre-activation anywhere near the kink; the negative channel is all negative: y and dx are exactly 0 there, in the restatement too
    pre = (inp["x"].double() - ref["mean"]) * ref["rstd"] * inp["gamma"].double() + inp["beta"].double()
    assert float(pre.abs().min()) > 1.0 and bool((pre[:, D.NEG_CH] < 0).all()) and bool((pre[:, [c for c in range(D.REGIME_C) if c != D.NEG_CH]] > 0).all())
    rst = D.bn_math(inp, F32)
    assert float(ref["dx"][:, D.NEG_CH].abs().max()) == 0 == float(rst["dx"][:, D.NEG_CH].abs().max()) and float(rst["y"][:, D.NEG_CH].abs().max()) == 0
    var = inp["x"].double().var(0, unbiased=False)
    assert D.rel_err(ref["rstd"], (var + D.BN_EPS).rsqrt()) < 1e-9
    if name == "mean_1e4":
        assert float((ref["mean"] - 1e4).abs().max()) < (0.2 if rows > 5 else 2) and 0.05 < float(var.min()) and float(var.max()) < 3
    if name == "constant":
        for ch, v in zip(D.CONST_CH, D.CONSTANTS):
            assert float(var[ch].abs()) < 1e-15 and float(ref["mean"][ch]) == v and abs(float(ref["rstd"][ch]) - D.BN_EPS ** -0.5) < 1e-9
            assert torch.equal(ref["y"][:, ch], inp["beta"][ch].double().expand(rows)) and torch.equal(rst["y"][:, ch], ref["y"][:, ch])
    if name == "one_row":           # count 1: the unbiased variance is the biased one (0), so running_var only decays
        assert rows == 1 and float(var.abs().max()) < 1e-15 and D.rel_err(ref["rvar"], 0.9 * inp["rvar"].double()) < 1e-7
        assert torch.equal(ref["mean"], inp["x"][0].double()) and float(ref["dx"].abs().max()) == 0 == float(rst["dx"].abs().max())


@pytest.mark.parametrize("rows", [2400, 5])
def test_a_one_pass_variance_misses_the_bound_tenfold(rows):
    """mean / std = 1e4: E[x^2] - E[x]^2 from f32 sums is at least 10 x outside the bounds of rstd, y and dx -- a statistics path without the centred second
    pass cannot pass the regime"""
    case = D.regime_case("mean_1e4", rows)
    bad = D.bn_errs(D.bn_math(case["inp"], F32, one_pass=True), case["ref"])
    for k in ("rstd", "y", "dx"):
        assert bad[k] >= D.ONE_PASS_FACTOR * case["bound"][k], (k, bad[k], case["bound"][k])


# ------------------------------------------------------------------------------------------------ C: lin_range covers lin_index
def _pairs():
    return sorted({(a, b) for a in range(1, 65) for b in range(1, 65)} | {(a, b) for a in D.Z for b in D.Z})


def test_lin_range_covers_every_output_with_a_weight():
    """For all (in, out) up to 64 and all of Z^2: every output o that resize_common.h:lin_index gives a non-zero weight for source i lies inside the
    [lo, hi] of decode_head.hip:lin_range, both restated in numpy float32, with and without the contraction of a * b - c into an fma (the build leaves
    -ffp-contract at hipcc's default, which contracts).  The build passes neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt, so the
    device's f32 division is the correctly rounded one; the enumeration is repeated with `inv` one ulp either way all the same.  The smallest slack
    of the unclamped bounds is printed; the margin of one is what it consists of: without the margin the cover still holds at these sizes, by a
    slack of zero -- so the mutation `margins removed` must be caught by values, and tests/test_hip_decode_edges.py says which."""
    worst = {}
    for fma in (False, True):
        for ulps in (0, -1, 1):
            slack = 1 << 30
            for a, b in _pairs():
                missed, s = D.range_cover(a, b, fma, ulps)
                assert missed == 0, "in %d -> out %d (fma %s, inv %+d ulp): %d weighted outputs outside lin_range" % (a, b, fma, ulps, missed)
                slack = min(slack, s)
            worst[(fma, ulps)] = slack
    print("lin_range: smallest slack of the unclamped bounds over %d pairs: %s" % (len(_pairs()), worst))
    assert min(worst.values()) >= 0
    assert all(set(D.seg_label_sizes(n)) <= set(D.Z) and min(D.seg_label_sizes(n)) <= n <= max(D.seg_label_sizes(n)) and len(D.seg_label_sizes(n)) >= 5 for n in D.Z)
    for n in D.Z[1:-1]:
        assert any(m < n for m in D.seg_label_sizes(n)) and any(m > n for m in D.seg_label_sizes(n))


@pytest.mark.parametrize("along_w", [True, False], ids=["W", "H"])
@pytest.mark.parametrize("n_in", D.Z)
def test_the_resize_inputs_leave_the_f32_index_rule_room_inside_the_tolerance(n_in, along_w):
    """what the GPU test's 1e-5 takes for granted: on its very inputs the f32 index arithmetic (exact sums otherwise) is within a quarter of the tolerance
    of float64 F.interpolate and autograd, contracted or not -- and a quarter of the loss's tolerances for the label sizes the gather is run at"""
    for n_out in D.Z:
        c = D.resize_case(n_in, n_out, along_w)
        assert torch.equal(c["x"].float().double(), c["x"]) and torch.equal(c["dy"].float().double(), c["dy"]) and torch.equal(c["dyb"].to(BF16).double(), c["dyb"])
        for fma in (False, True):
            y, dx = D.resize_restated(n_in, n_out, along_w, fma)
            assert D.rel_err(y, c["y"]) < D.TOL_FWD / 4 and D.rel_err(dx, c["dx"]) < D.TOL_FWD / 4, (n_out, fma, D.rel_err(y, c["y"]), D.rel_err(dx, c["dx"]))
    for m in D.seg_label_sizes(n_in):
        c = D.seg_ratio_case(n_in, m, along_w)
        for fma in (False, True):
            loss, dl = D.seg_ratio_restated(n_in, m, along_w, fma)
            assert abs(float(loss - c["loss"])) < D.TOL_LOSS / 4 * float(c["loss"]) and D.rel_err(dl, c["dlogits"]) < D.TOL_DLOGITS / 4, (m, fma)


def test_the_numpy_restatement_is_the_index_rule_of_interpolate():
    """lin_index_np against float64 F.interpolate: the weights it gives reproduce torch's forward on an identity-like probe"""
    for a, b in [(1, 7), (7, 1), (5, 13), (255, 256), (256, 255), (513, 3), (3, 513), (64, 65)]:
        i0, i1, w0, w1 = D.lin_index_np(a, b)
        x = torch.randn(1, 1, 1, a, dtype=F64, generator=torch.Generator().manual_seed(a + b))
        want = F.interpolate(x, size=(1, b), mode="bilinear", align_corners=False)[0, 0, 0]
        got = x[0, 0, 0][torch.from_numpy(i0)] * torch.from_numpy(w0.astype(np.float64)) + x[0, 0, 0][torch.from_numpy(i1)] * torch.from_numpy(w1.astype(np.float64))
        assert D.rel_err(got, want) < 1e-4, (a, b)                              # (random neighbours: the f32 position's own rounding shows; a wrong index is O(1))
    src = source("resize_common.h") + source("decode_head.hip")
    for line in ("float src = scale * ((float)o + 0.5f) - 0.5f;", "const float inv = (float)out / (float)in;", "lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;",
                 "hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;", "if (i == in - 1) hi = out - 1;"):
        assert line in src, line


def test_a_bound_one_short_would_lose_a_contribution_at_these_sizes():
    """the enumeration can see a short bound: with the margin at -1 (one short on each side) weighted outputs fall outside at the sizes of Z"""
    assert sum(D.range_cover(a, b, False, 0, margin=-1)[0] for a in D.Z for b in D.Z) > 0
    assert D.range_cover(5, 255, False, 0, margin=-1)[0] > 0 and D.range_cover(3, 21, True, 0, margin=-1)[0] > 0


# ------------------------------------------------------------------------------------------------ D .. F: the cases are what they are named for
def test_the_loss_cases_are_what_their_names_say():
    c = {n: D.seg_case(n) for n in D.SEG_CASES}
    for n, k in c.items():
        assert bool(torch.isfinite(k["loss"])) and bool(torch.isfinite(k["dlogits"]).all()), n
        assert torch.equal(k["logits"].to(k["dtype"]).float(), k["logits"]), n
        kept = k["labels"] != k["ignore_index"]
        assert bool(((k["labels"] >= 0) & (k["labels"] < k["K"]))[kept].all()), n
        assert torch.equal(k["labels"].to(k["label_dtype"]).long(), k["labels"]), n            # the label type holds every label and the ignore index
    assert c["bf16_u8"]["dtype"] == c["bf16_i64"]["dtype"] == BF16 and {c["bf16_u8"]["label_dtype"], c["bf16_i64"]["label_dtype"]} == {torch.uint8, torch.int64}
    assert float(c["one_hot"]["logits"].abs().min()) == 3e4 and 1e3 < float(c["one_hot"]["loss"]) < 6e4 * 0.7
    t = c["near_ties"]["logits"]
    assert float(t.abs().max()) > 3e4 and float(t.abs().min()) >= 3e4 - 2 and float((t.max(1)[0] - t.min(1)[0]).max()) <= 2.0 and float(c["near_ties"]["loss"]) > 0.1
    assert c["k1"]["K"] == 1 and float(c["k1"]["loss"]) == 0 and float(c["k1"]["dlogits"].abs().max()) == 0 and bool((c["k1"]["labels"] == 0).any())
    assert c["k4096"]["K"] == D.SEG_K_MAX == 4096 and tuple(c["k4096"]["labels"].shape) == (1, 2, 2)
    assert c["ignore_neg100"]["ignore_index"] == -100 and c["ignore_neg100"]["label_dtype"] == torch.int64 and bool((c["ignore_neg100"]["labels"] == -100).any())
    assert bool((c["all_ignored"]["labels"] == -100).all()) and float(c["all_ignored"]["loss"]) == 0 and float(c["all_ignored"]["dlogits"].abs().max()) == 0
    m = c["many_partials"]
    assert m["N"] * m["H"] * m["W"] == 66049 and -(-66049 // 256) == 259 > 256
    assert (c["ragged"]["N"] * c["ragged"]["H"] * c["ragged"]["W"]) % 256 == 21
    assert c["coarse_labels"]["H"] < c["coarse_labels"]["h"] and c["coarse_labels"]["W"] < c["coarse_labels"]["w"]
    r = D.logit_rows(c["ragged"]["logits"])
    assert r.shape[1] == 24 and bool(torch.isnan(r[:, 19:]).all()) and not bool(torch.isnan(r[:, :19]).any())
    # the reference is torch_seg_loss
    from test_uper_head import torch_seg_loss
    k = c["coarse_labels"]
    assert torch.equal(torch_seg_loss(k["logits"].double(), k["labels"], k["ignore_index"], 0.7), k["loss"])


def test_the_tile_and_mask_cases_sit_on_their_seams():
    T = D.FUSE_TILE
    (a, b, c, d) = D.FUSE_SHAPES
    S = [s[2] * s[3] for s in D.FUSE_SHAPES]
    assert S[0] == 68 and S[0] % 4 == 0 and S[0] % T == 4 and a[1] % T == 4                      # vectorised, 4 positions and 4 channels in the second tiles
    assert S[1] == 65 and S[1] % 4 != 0 and b[1] == 2 * T + 4                                    # scalar, a third channel tile of 4
    assert S[2] == T and c[1] == 4                                                                 # exactly one tile of positions
    assert d[0] // 2 == 3 and S[3] % 4 == 0                                                        # N = 3: b % N and b / N differ for b = 1 .. 5 but b = 4
    assert [(b_ % 3, b_ // 3) != (b_ // 3, b_ % 3) for b_ in range(6)].count(True) >= 4
    assert (D.FUSE_OFFSET_SHAPE[2] * D.FUSE_OFFSET_SHAPE[3]) % 4 == 0                              # only the base's alignment keeps it off the vector kernel
    assert "const bool vec = (S % 4) == 0 && ((uintptr_t)f & 15) == 0;" in source("unet_head.hip")
    assert any(hs > 2 * h for h, w, hs, ws in D.UP_CASES) and any(ws > 2 * w for h, w, hs, ws in D.UP_CASES)      # the skip is LARGER than the output: the downscale branch
    assert any(hs < 2 * h and ws < 2 * w for h, w, hs, ws in D.UP_CASES)
    assert all(S_ == D.POOL_S_MAX for _, _, S_ in D.POOL_CASES) and {(H >= 64, W >= 64) for H, W, _ in D.POOL_CASES} == {(True, True), (True, False), (False, False)}
    for rps in D.CS_RPS:
        for C in D.CS_C:
            x, mask, ref = D.channel_scale_case(rps, C)
            assert set(mask.unique().tolist()) == {0.0, 2.0} and len({tuple(r.tolist()) for r in mask}) == D.CS_N and float(x.abs().min()) > 0
            assert torch.equal(x.to(BF16).float(), x) and torch.equal(ref.to(BF16).float(), ref)
            # r % rows_per_sample instead of r / rows_per_sample gives another result at every size (rows_per_sample = 1 included: row 0 for all)
            rows = torch.arange(D.CS_N * rps)
            assert not torch.equal(x * mask[(rows % rps) % D.CS_N], ref)
    assert (D.CS_C[1] // 4) % 64 == 1 and 3 * 65 * (D.CS_C[1] // 4) > 256 * 48


# ------------------------------------------------------------------------------------------------ refusals
def _check_lines(entry, text):
    """the MTP_CHECK_ARG lines of `entry` up to and including the one that holds `text`"""
    src = source("decode_head.hip").split("\n")
    start = [i for i, l in enumerate(src) if l.startswith('extern "C"') and (entry + "(") in l]
    assert len(start) == 1
    lines = []
    for l in src[start[0]:]:
        if "MTP_CHECK_ARG" in l:
            lines.append(l)
            if text in l:
                return lines
        assert not l.startswith("}"), "%s has no check %r" % (entry, text)


def test_every_refusal_is_refused_by_the_check_it_names():
    """K = 4097 and S = 65 pass every conjunct of their entry's argument checks but the named one (the same call with K = 4096 / S = 64 in the restated
    conjuncts passes them all), and the library itself returns MTP_ERR_ARG before it touches a pointer (P is never dereferenced)"""
    from mtp_amd import _lib
    L, P = lib(), 1 << 20
    ERR_ARG = -1
    with pytest.raises(_lib.MtpHipError, match=D.ERR_ARG_TEXT % "mtp_seg_ce"):
        _lib.check(ERR_ARG, "mtp_seg_ce")
    # mtp_seg_ce: the first check holds K <= 4096; every other conjunct of it is true for the call
    lines = _check_lines(*D.REFUSALS["seg_ce_k4097"][:2])
    assert len(lines) == 1 and re.sub(r"\s+", " ", lines[0]).strip() == \
        "MTP_CHECK_ARG(logits && labels && loss && dlogits && workspace && N > 0 && h > 0 && w > 0 && K > 0 && K <= 4096 && H > 0 && W > 0);"
    for K, want in ((4097, ERR_ARG),):
        ws = L.mtp_seg_ce_workspace_bytes(1, 2, 2, K)
        assert ws == (4 * K + 1) * 4
        assert L.mtp_seg_ce(P, 0, K, 1, 1, 2, K, P, 8, 2, 2, 255, 1.0, P, P, K, P, ws, None) == want
    for entry, args in (("pool_fwd_s65", lambda S: (P, 0, 8, P, 0, 1, 65, 63, 8, S, None)), ("pool_bwd_s65", lambda S: (P, 0, P, 8, 1, 65, 63, 8, S, 0, None))):
        name, text, _ = D.REFUSALS[entry]
        lines = _check_lines(name, text)
        assert len(lines) == 1 and "S > 0 && S <= 64" in lines[0] and "N > 0 && H > 0 && W > 0 && C > 0 && (C % 4) == 0" in lines[0]
        assert getattr(L, name)(*args(65)) == ERR_ARG
