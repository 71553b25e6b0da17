"""CPU: the inputs of tests/test_hip_det_edges.py meet their conditions (tests/det_edge_cases.py, from the float64 references alone), the exact cases
are exact (the float32 and the float64 run of the reference coincide bit for bit), every exact cut-off case changes when a cut-off comparison is
flipped, and what det_edge_cases and rpn_ref add to the references agrees with what was there.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import det_edge_cases as D
import roi_cases as RC
import roi_ref as R
import rpn_cases as PC
import rpn_ref as PR
from mtp_amd import _lib, ops

F64, F32 = np.float64, np.float32
SIZES128 = RC.sizes_of((128, 128))


# ------------------------------------------------------------------------------------------------------------------- 1. RoIAlignRotated
def test_committed_seeds_are_the_first_that_pass():
    found = D.find_seeds()
    assert found["GEOM"] == D.GEOM_SEEDS and found["PIXEL"] == D.PIXEL_SEED and found["CLAMP"] == D.CLAMP_SEED
    assert found["LOSS"] == D.LOSS_SEEDS and found["PREDICT"] == D.PREDICT_SEEDS and found["PROP"] == D.PROP_SEEDS


def test_wide_and_geometry_cases_meet_their_conditions():
    assert [-(-c // 64) for c in D.WIDE_C] == [1, 2, 3] and 65 % 64 == 1      # gridDim.y of the gather; one live lane in the second block
    for c in D.WIDE_C:
        maps, rois = D.wide_case(c)
        assert RC.align_condition((None, rois)) and len(rois) == 24 and [m.shape for m in maps] == [(D.BATCH, c, H, W) for H, W in SIZES128]
    assert {(p, s) for p, s, _ in D.GEOMS} == {(1, 1), (7, 1), (7, 3), (3, 2), (14, 2), (8, 4), (16, 2), (32, 1)}
    assert sum(p * p * s * s == ops.ROI_MAX_POINTS for p, s, _ in D.GEOMS) == 3 and len({(p, s) for p, s, cw in D.GEOMS if not cw} & {(p, s) for p, s, cw in D.GEOMS if cw}) >= 2
    for g in D.GEOMS:
        maps, rois = D.geom_case(*g)
        assert D.geom_condition(rois, *g) and len(rois) == 12
    assert all(p * p * s * s > ops.ROI_MAX_POINTS for p, s in D.GEOM_REFUSED)


def test_backward_by_add_at_is_roi_ref_backward():
    """det_edge_cases.roi_align_bwd adds the same products in the same order as roi_ref.roi_align_bwd: the same bits, in both precisions"""
    maps, rois = RC.align_case()
    shapes = [m.shape for m in maps[RC.C]]
    dout = np.random.default_rng(1).normal(0, 1, (len(rois), RC.C, RC.P, RC.P)).astype(F32)
    valid = np.arange(len(rois)) % 5 != 2
    for dtype in (F64, F32):
        for kw in (dict(), dict(valid=valid), dict(levels=(R.map_levels(rois, 4, RC.FINEST) + 1) % 4)):
            a = R.roi_align_bwd(dout, shapes, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, dtype=dtype, **kw)
            b = D.roi_align_bwd(dout, shapes, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, dtype=dtype, **kw)
            assert all(x.dtype == y.dtype == dtype and np.array_equal(x, y) for x, y in zip(a, b)) and any(x.any() for x in a)
    rois, dout = D.hot_case()      # thousands of additions into one pixel
    for dtype in (F64, F32):
        a = R.roi_align_bwd(dout[::12], [(2, D.HOT_C, 32, 32)], rois[::12], RC.STRIDES[:1], RC.P, RC.S, True, dtype=dtype)
        b = D.roi_align_bwd(dout[::12], [(2, D.HOT_C, 32, 32)], rois[::12], RC.STRIDES[:1], RC.P, RC.S, True, dtype=dtype)
        assert np.array_equal(a[0], b[0])


def test_exact_cutoff_case_is_exact_and_discriminates():
    maps, rois, dout = D.exact_case()
    P, S, st = D.EXACT_P, D.EXACT_S, (D.EXACT_STRIDE,)
    lv = np.zeros(len(rois), np.int64)
    want = {0: (np.arange(-1, 7), np.arange(-1, 7)), 1: (np.arange(1, 9), np.arange(1, 9)), 2: (np.arange(-1, 7), np.arange(1, 9)), 3: (np.arange(1, 9), np.arange(-1, 7)),
            4: (np.arange(0.5, 8), np.arange(-0.5, 7))}
    for cw in (True, False):
        for r, (ys, xs) in want.items():      # the samples sit where intended, in both precisions
            for dtype in (F64, F32):
                y, x = R.sample_points(rois[r], 8, 8, 0.25, P, S, cw, dtype)
                y, x = y.reshape(P, P, S, S), x.reshape(P, P, S, S)
                assert y.dtype == dtype and np.array_equal(y.transpose(0, 2, 1, 3).reshape(8, 8), np.repeat(ys[:, None], 8, 1))
                assert np.array_equal(x.transpose(0, 2, 1, 3).reshape(8, 8), np.repeat(xs[None, :], 8, 0))
                assert R.bilinear(y, x, 8, 8, dtype)[0].all()      # all 64 counted inside
        f64 = R.roi_align(maps, rois, st, P, S, cw, levels=lv)
        f32 = R.roi_align(maps, rois, st, P, S, cw, levels=lv, dtype=F32)
        assert D.same32(f64, f32) and np.abs(f64).max() > 1
        assert np.array_equal(R.roi_align(maps, rois, st, P, S, cw), f64)      # the computed level is level 0 too
        closed = D.roi_align_cut(maps, rois, st, P, S, cw, lv)
        assert np.array_equal(closed, f64) and D.same32(closed, D.roi_align_cut(maps, rois, st, P, S, cw, lv, dtype=F32))
        lo, hi = D.roi_align_cut(maps, rois, st, P, S, cw, lv, lo_open=True), D.roi_align_cut(maps, rois, st, P, S, cw, lv, hi_open=True)
        changed = lambda a: [bool((a[r] != f64[r]).any()) for r in range(len(rois))]      # noqa: E731
        assert changed(lo) == [True, False, True, True, False] and changed(hi) == [False, True, True, True, False]
        # the -1 row with the W column: the first bin row changes under `y > -1`, the last bin column under `x < W`, and only those
        assert (lo[2] != f64[2]).any((0, 2)).tolist() == [True, False, False, False] and (hi[2] != f64[2]).any((0, 1)).tolist() == [False, False, False, True]
        shapes = [m.shape for m in maps]
        g64, g32 = D.roi_align_bwd(dout, shapes, rois, st, P, S, cw, levels=lv), D.roi_align_bwd(dout, shapes, rois, st, P, S, cw, levels=lv, dtype=F32)
        assert D.same32(g64[0], g32[0]) and np.array_equal(g64[0], R.roi_align_bwd(dout, shapes, rois, st, P, S, cw, levels=lv)[0]) and g64[0].any()
    # the pixel H - 1 = 7 is reached through the clamp branch (yl >= H - 1) and row 0 through the clamp of negatives
    y, x = D.exact_samples(rois[1], True)
    _, (yl, yh, xl, xh), w = R.bilinear(y, x, 8, 8)
    assert yl.max() == yh.max() == 7 and set(yl[y >= 7]) == {7} and all((wk == 0).all() for wk in (w[1], w[2], w[3]))      # integer pixels: zero high weights


def test_pixel_slot_and_hot_cases_meet_their_conditions():
    assert D.pixel_condition(D.pixel_case()) and sorted(set(D.pixel_case()[1].tolist())) == [0, 1, 2]
    # slots: the finite ones keep CUT_GAP under their stated levels; the level map of those whose product is a positive number keeps LEVEL_GAP
    rois, lv = D.SLOT_ROIS, D.SLOT_LEVELS
    fin = D.SLOT_FINITE
    assert D.margins_ok(rois[fin], lv[fin], SIZES128, D.STRIDES, RC.P, RC.S, True, computed=False)
    prod = rois[:, 3].astype(F64) * rois[:, 4]
    named = [i for i in fin if prod[i] > 0]
    assert named == [0, 1, 2, 3, 13] and (R.level_margin(rois[named], D.FINEST) > D.LEVEL_GAP).all()
    assert R.map_levels(rois[named], 4, D.FINEST).tolist() == lv[named].tolist() and not lv[[i for i in range(len(rois)) if i not in named]].any()
    assert (D.SLOT_LEVELS_OUT[D.SLOT_BAD_IMAGE] == -1).all() and not D.SLOT_LEVELS_OUT[D.SLOT_NAN_SIZE].any() and D.slot_valid().sum() == len(fin)
    clamped = np.clip(D.SLOT_OVERRIDE, 0, 3)
    assert clamped.tolist() == [0, 3, 0, 3] and D.margins_ok(rois[:4], clamped, SIZES128, D.STRIDES, RC.P, RC.S, True, computed=False)
    ref = R.roi_align(D.geom_maps(), D.slot_rois_for_ref(), D.STRIDES, RC.P, RC.S, True, D.FINEST, levels=lv, valid=D.slot_valid())
    assert all(ref[i].any() for i in fin) and not ref[~D.slot_valid()].any()      # zero and negative sizes still read the map
    # hot pixel: each RoI touches 2 x 2 pixels of level 0, two of them shared; 48 copies x 196 samples a pixel
    rois, dout = D.hot_case()
    assert len(rois) == 2 * D.HOT_COPIES and (R.map_levels(rois, 4, D.FINEST) == 0).all() and (R.level_margin(rois, D.FINEST) > D.LEVEL_GAP).all()
    px = []
    for r in D.HOT_ROIS:
        y, x = R.sample_points(r, 32, 32, 0.25, RC.P, RC.S, True)
        _, (yl, yh, xl, xh), _ = R.bilinear(y, x, 32, 32)
        px.append({(int(a), int(b)) for a, b in zip(np.concatenate([yl.ravel(), yh.ravel()]), np.concatenate([xl.ravel(), xh.ravel()]))} |
                  {(int(a), int(b)) for a, b in zip(np.concatenate([yl.ravel(), yh.ravel()]), np.concatenate([xh.ravel(), xl.ravel()]))})
    assert px[0] == {(7, 10), (7, 11), (8, 10), (8, 11)} and px[1] == {(7, 11), (7, 12), (8, 11), (8, 12)} and len(px[0] & px[1]) == 2
    maps, roi, dout = D.small_case()
    assert maps[0].shape == (1, 1, 6, 5) and D.margins_ok(roi, [0], [(6, 5)], (D.SMALL_STRIDE,), RC.P, RC.S, True, computed=False)
    assert R.roi_align(maps, roi, (D.SMALL_STRIDE,), RC.P, RC.S, True, levels=[0]).all()      # wholly inside the map
    assert D.HOT_COPIES * RC.P * RC.P * RC.S * RC.S * 2 > 4 * 256 * 4     # a run of equal keys spans many workgroups of the gather (4 positions each)


# ------------------------------------------------------------------------------------------------------------------- 2. RoI loss and predict
def test_loss_cases_meet_their_conditions():
    assert {c[0] for c in D.LOSS_CASES} == {1, 255, 256, 257, 512, 600} and {c[2] for c in D.LOSS_CASES} == {1, 5, 15, 80} and (512, 2, 15, 3) in D.LOSS_CASES
    assert {c[1] for c in D.LOSS_CASES} == {1, 2, 3} and {c[3] for c in D.LOSS_CASES} == {0, 3}
    kinds = set()
    for S, B, K, _ in D.LOSS_CASES:
        c = D.loss_case(S, B, K)
        assert D.loss_condition(c) and c["cls"].shape == (B * S, K + 1)
        used = c["n_pos"] + c["n_neg"]
        assert (used <= S).all() and (c["n_pos"] >= 0).all()
        kinds |= {"full"} if (used == S).any() else set()
        kinds |= {"partial"} if ((used > 0) & (used < S)).any() else set()
        kinds |= {"zero"} if (used == 0).any() else set()
        kinds |= {"no_pos"} if ((c["n_pos"] == 0) & (used > 0)).any() else set()
        kinds |= {"partial_in_second_chunk"} if ((used > 257) & (used < S)).any() else set()
        kinds |= {"one_live_thread"} if S == 257 and (used == S).any() else set()
    assert kinds == {"full", "partial", "zero", "no_pos", "partial_in_second_chunk", "one_live_thread"}


def test_clamp_case_and_its_cleaned_lists():
    assert D.clamp_condition(D.CLAMP_SEED)
    c, given, clean = D.clamp_case()
    S = D.CLAMP_S
    assert D.clamp_counts([-4, S + 9, 10, 3], [12, 3, S, -1], S)[0].tolist() == [0, S, 10, 3] and D.clamp_counts([-4, S + 9, 10, 3], [12, 3, S, -1], S)[1].tolist() == [12, 0, S - 10, 0]
    assert given["sample_gt"][3, 6] == -1 and given["sample_gt"][3, 7] == D.NUM_G and given["n_pos"][3] == 8      # the last two positives name no gt
    assert sorted(set(given["gt_labels"].tolist()) - set(range(D.CLAMP_K))) == [-2, D.CLAMP_K + 3] and (clean["gt_labels"] <= D.CLAMP_K).all() and (clean["gt_labels"] >= 0).all()
    hit = clean["sample_gt"][:3].reshape(-1)      # both out-of-range labels are met by a positive, so the box term under a background label is compared
    ref = D.loss_ref(c, **clean)
    pos = np.concatenate([b * S + np.arange(clean["n_pos"][b]) for b in range(4)])
    labels_of_pos = clean["gt_labels"][clean["sample_gt"].reshape(-1)[pos]]
    assert (labels_of_pos == D.CLAMP_K).any() and ref["dreg"][pos][labels_of_pos == D.CLAMP_K].any() and len(hit)
    assert int(ref["labels"][3 * S + 6]) == int(ref["labels"][3 * S + 7]) == D.CLAMP_K and not ref["dreg"][3 * S + 6:3 * S + 8].any() and ref["dcls"][3 * S + 6:3 * S + 8].any()


def test_softmax_regimes_and_kinks_are_exact_where_they_say():
    for name, (c, exact) in D.softmax_cases().items():
        r64, r32 = D.loss_ref(c), D.loss_ref(c, F32)
        if exact:
            assert all(D.same32(np.asarray(r64[k], F64), np.asarray(r32[k], F32)) for k in ("loss_cls", "loss_bbox", "acc", "dcls", "dreg")), name
    c = D.softmax_cases()["ahead200"][0]
    r = D.loss_ref(c)
    assert float(r["loss_cls"]) == 100.0 and float(r["acc"]) == 50.0 and float(r["loss_bbox"]) == 0.0      # (0 + 200 + 0 + 200) / 4
    want = np.zeros((4, 6), F32)
    want[1, 4], want[1, 0], want[3, 1], want[3, 5] = 0.25, -0.25, 0.25, -0.25      # the wrong rows: p - onehot over 4 samples
    assert np.array_equal(r["dcls"].astype(F32), want)
    eq0, eq3 = (D.loss_ref(D.softmax_cases()[k][0]) for k in ("equal_label0", "equal_label3"))
    assert float(eq0["acc"]) == 50.0 and float(eq3["acc"]) == 0.0 and abs(float(eq0["loss_cls"]) - np.log(6)) < 1e-12      # ties: the argmax is index 0
    for beta in D.KINK_BETAS:
        for f in D.KINK_FACTORS:
            c = D.kink_case(beta, f)
            lb, dr = D.kink_expected(beta, f)
            r64, r32 = D.loss_ref(c, beta=beta), D.loss_ref(c, F32, beta=beta)
            assert not r64["targets"].any() and not r32["targets"].any()      # prior = gt at theta 0: every target exactly 0
            assert r32["loss_bbox"].dtype == F32 and r32["loss_bbox"] == lb and np.array_equal(r32["dreg"][0], dr), (beta, f)
            assert D.same32(np.asarray(r64["loss_bbox"]), np.asarray(r32["loss_bbox"])) and D.same32(r64["dreg"], r32["dreg"])
    assert float(D.kink_expected(1.0, 1.0)[0]) == 2.5 and float(D.kink_expected(1.0, 0.0)[0]) == 0 and D.kink_expected(0.25, -1.0)[1].tolist() == [-1.0] * 5
    assert float(D.kink_expected(1.0, 1 - 2.0 ** -20)[1][0]) == 1 - 2.0 ** -20 and float(D.kink_expected(0.25, 1 + 2.0 ** -20)[1][0]) == 1.0


def test_predict_cases_meet_their_conditions():
    assert {c[0] for c in D.PREDICT_CASES} == {1, 255, 256, 257, 1000} and {c[1] for c in D.PREDICT_CASES} == {1, 15, 80}
    for n, K, _ in D.PREDICT_CASES:
        c = D.predict_case(n, K)
        assert D.predict_condition(c, n) and c["cls"].shape == (n, K + 1)
        sc = R.softmax(c["cls"])[:, :K]
        assert (sc > D.SCORE_THR).any() and ((sc < D.SCORE_THR).any() or K == 1)      # the threshold divides the table


# ------------------------------------------------------------------------------------------------------------------- 3. the oriented RPN
def test_rpn_seam_cases():
    priors, inside, sizes = PC.anchors(D.RPN_NAME)
    for S in D.RPN_S:
        c = D.rpn_seam_case(S)
        for b in range(D.BATCH):
            assert len(set(c["samples"][b].tolist())) == S and inside[c["samples"][b]].all()      # inside anchors, without repeats
            assert (c["sample_gt"][b, :c["n_pos"][b]] >= 0).all() and c["n_pos"][b] + c["n_neg"][b] <= S
        per = D.rpn_seam_levels(c, S)
        assert (per.sum(1) == 0).any()      # a level without a sample
        if S > 256:
            assert per.shape[1] >= 2 and ((per > 0).sum(1) >= 2).any()      # a level with samples from more than one chunk
        assert int(c["n_pos"][0] + c["n_neg"][0]) == S      # S = 257: the full image has the one live thread of the second chunk
    assert PC.corner_condition(np.concatenate(PC.case(D.RPN_NAME)[2]))      # the encode's 0.1 cut depends on the gts alone


def test_rpn_ref_extensions():
    """avg_factor and the gt row -1 of rpn_ref.loss: the defaults are what they were (tests/test_rpn_host.py holds them against fixture f22)"""
    c = D.rpn_seam_case(255)
    base = D.rpn_loss_ref(c)
    n = int(c["n_pos"].sum() + c["n_neg"].sum())
    same = D.rpn_loss_ref(c, avg_factor=n)
    assert all(np.array_equal(a, b) for a, b in zip(base[:2], same[:2])) and all(np.array_equal(a, b) for a, b in zip(base[2] + base[3], same[2] + same[3]))
    half = D.rpn_loss_ref(c, avg_factor=2 * n)      # a power of two: exactly half
    assert all(np.array_equal(a, 2 * b) for a, b in zip(base[:2], half[:2])) and all(np.array_equal(a, 2 * b) for a, b in zip(base[2] + base[3], half[2] + half[3]))
    d = dict(c, pgt=[np.concatenate([[-1], c["pgt"][0][1:]]), c["pgt"][1]])      # the first positive of image 0 names no gt
    cut = D.rpn_loss_ref(d)
    assert np.array_equal(cut[0], base[0]) and all(np.array_equal(a, b) for a, b in zip(cut[2], base[2]))      # the classification is untouched
    l, y, x, a = (int(v[0]) for v in PR.level_of(c["pos"][0][:1], PC.anchors(D.RPN_NAME)[2], PC.A))
    assert base[3][l][0, a * 6:a * 6 + 6, y, x].any() and not cut[3][l][0, a * 6:a * 6 + 6, y, x].any() and cut[1][l] < base[1][l]
    zeroed = [g.copy() for g in base[3]]
    zeroed[l][0, a * 6:a * 6 + 6, y, x] = 0
    assert all(np.array_equal(g, z) for g, z in zip(cut[3], zeroed))
    given, clean, avg = D.rpn_bad_case()
    assert avg == 26 + D.RPN_BAD_S and [len(p) for p in clean["pos"]] == [5, D.RPN_BAD_S] and [len(p) for p in clean["neg"]] == [19, 0] and (clean["pgt"][0] == -1).sum() == 1
    K = sum(len(g) for g in PC.case(D.RPN_NAME)[2])
    assert given["samples"][0, 2] == -1 and given["samples"][0, 9] == len(PC.anchors(D.RPN_NAME)[0]) and given["sample_gt"][0, 4] == K and given["n_pos"][1] > D.RPN_BAD_S


def test_proposal_cases_meet_their_conditions():
    for name in D.PROP_SHAPES:
        c = D.prop_case(name)
        assert D.prop_condition(c) and c["A"] == D.PROP_SHAPES[name][0]
        counts = [H * W * c["A"] for H, W in c["sizes"]]
        assert len(c["priors"]) == sum(counts) and all(len(set(k.tolist())) == len(k) for kb in c["keep"] for k in kb)
        if len(counts) == 3:
            assert c["keep_counts"][1] == 0 and c["keep_counts"][2] == counts[2] and 0 < c["keep_counts"][0] < counts[0]
    assert {D.PROP_SHAPES[n][0] for n in D.PROP_SHAPES} >= {1, 9} and len(D.PROP_SHAPES["single"][1]) == 1


# ------------------------------------------------------------------------------------------------------------------- the limit, stated twice
def test_point_limit_of_wrapper_and_library_flip_together():
    """ops.ROI_MAX_POINTS and kMaxEntries of csrc/roi_head.hip (four corner entries a point) are one limit: beyond it the wrapper raises and the
    library answers MTP_ERR_ARG before it launches (the pointers below are never dereferenced); up to it the wrapper accepts, and
    tests/test_hip_det_edges.py runs the three geometries that sit on it through both"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "roi_head.hip")).read()
    k_max = int(re.search(r"constexpr int kMaxEntries = (\d+);", src).group(1))
    assert k_max == 4 * ops.ROI_MAX_POINTS == 4096
    lib = _lib.load()
    Pp = 1 << 20
    lv = (_lib.RoiLevel * 1)()
    lv[0].map, lv[0].dmap, lv[0].H, lv[0].W, lv[0].spatial_scale = Pp, Pp, 8, 8, 0.25
    rois = torch.zeros(4, 6)
    beyond = 0
    for p in range(1, 41):
        for s in range(1, 9):
            over = p * p * s * s * 4 > k_max
            if over:
                beyond += 1
                with pytest.raises(ValueError):
                    ops._roi_check("t", rois, None, None, p, s)
                assert lib.mtp_roi_align_rotated_fwd(lv, 1, 2, 8, Pp, None, None, 4, 0, p, s, 1, 56.0, Pp, None, None) == -1
                assert lib.mtp_roi_align_rotated_bwd_entries(lv, 1, 2, Pp, None, None, 4, 0, p, s, 1, 56.0, Pp, Pp, None) == -1
                assert lib.mtp_roi_align_rotated_bwd_gather(lv, 1, 2, 8, Pp, Pp, Pp, Pp, 4, p, s, 0, None) == -1
            else:
                assert ops._roi_check("t", rois, None, None, p, s) == (4, 0)
    assert beyond > 100 and (8, 5) in D.GEOM_REFUSED and (33, 1) in D.GEOM_REFUSED
    assert C.sizeof(_lib.RoiLevel) == 72
