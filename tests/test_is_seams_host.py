"""CPU: the conditions of tests/is_seam_cases.py, from the float64 restatements (mask_ref, hbox_ref) alone: what the seam tests of the
instance-segmentation kernels (tests/test_hip_is_seams.py) rely on must hold before a kernel runs.  Also mask_ref against the naive RoIAlign loop
at the sizes the existing host test does not reach, and the wrappers' refusals at the caps."""
import numpy as np
import pytest
import torch

import hbox_cases as HC
import is_seam_cases as SC
import mask_cases as MC
import mask_ref as MR
from mtp_amd import ops
from test_mask_host import naive_roi_align

F64, F32 = np.float64, np.float32


# ------------------------------------------------------------------------------------------------------------------- 1. RoIAlign chunks
def test_align_geometry_puts_the_boundaries_inside_workgroups():
    c = SC.align_case()
    per = [h * w for h, w in SC.AL_SIZES]
    image1, level1, pixels = per[0], SC.AL_IMAGES * per[0], SC.AL_IMAGES * sum(per)
    assert (image1, level1, pixels) == (35, 70, 82) and image1 % 4 == 3 and level1 % 4 == 2 and pixels % 4 == 2      # the last workgroup: two idle waves
    assert SC.AL_R == 130 and -(-SC.AL_R // 64) == 3 and SC.AL_R % 64 == 2                                                # trips of 64, 64 and 2
    rois, lv = c["rois"], c["levels"]
    assert (rois[:65, 0] == 0).all() and (rois[65:127, 0] == 1).all() and (rois[127:, 0] == 0).all()
    assert (lv[list(SC.AL_NAMED)] == 0).all() and set(lv[65:127].tolist()) == {0, 1} and lv.dtype == np.int32
    assert SC.AL_NAMED == (0, 63, 64, 127, 128, 129)      # lane 0 and lane 63 of the first two trips, both lanes of the last
    use = SC.align_in_use("valid")
    assert use.sum() == sum(SC.AL_COUNTS) and use[[0, 63, 64, 127, 128]].all() and not use[129] and not use[26:52].any()
    assert max(SC.AL_C) == SC.AL_CMAX and {1, 64, 65, 256, 257} == set(SC.AL_C)


def test_align_reference_of_fewer_channels_is_a_slice():
    """no operation of RoIAlign mixes channels: the reference at C channels is the first C channels of the reference at 257, bit for bit"""
    refs = SC.align_refs("all")
    for ft, kf, kb in ((F64, "fwd64", "bwd64"), (F32, "fwd32", "bwd32")):
        assert np.array_equal(SC._align_run(SC.SZ_C, None, ft, "fwd"), refs[kf][:, :SC.SZ_C])
        assert all(np.array_equal(a, b[:, :SC.SZ_C]) for a, b in zip(SC._align_run(SC.SZ_C, None, ft, "bwd"), refs[kb]))


@pytest.mark.parametrize("Cc", SC.AL_C)
def test_align_every_named_roi_weighs_on_the_pixel(Cc):
    """taking one of the named RoIs out of use moves the float64 gradient at pixel (3, 2) of image 0, level 0, in every channel, by at least 10 x the
    bound the GPU test holds that level to: a dropped lane or trip of the walk cannot pass"""
    refs = SC.align_refs("all")
    bound, e32 = SC.bound_of(refs["bwd64"][0][:, :Cc], refs["bwd32"][0][:, :Cc])
    full = refs["bwd64"][0][0, :Cc, SC.AL_PIXEL[0], SC.AL_PIXEL[1]]
    for r in SC.AL_NAMED:
        moved = np.abs(full - SC.align_without(r)[:Cc])
        print("C %d RoI %d: moved %.3e .. %.3e, bound %.3e" % (Cc, r, moved.min(), moved.max(), bound))
        assert moved.min() >= 10 * bound, (Cc, r, float(moved.min()), bound)
    for l in range(len(SC.AL_SIZES)):      # image 1 receives a gradient on both levels, in every channel
        assert (np.abs(refs["bwd64"][l][1, :Cc]).reshape(Cc, -1).max(1) > 10 * bound).all()
    assert np.abs(refs["fwd64"][list(SC.AL_NAMED)]).max() > 0.1


def test_align_valid_counts_weigh_too():
    refs, use = SC.align_refs("valid"), SC.align_in_use("valid")
    bound, _ = SC.bound_of(refs["bwd64"][0], refs["bwd32"][0])
    full = refs["bwd64"][0][0, :, SC.AL_PIXEL[0], SC.AL_PIXEL[1]]
    for r in SC.AL_NAMED:
        if use[r]:
            assert np.abs(full - SC.align_without(r, "valid")).min() >= 10 * bound, r
    assert not refs["fwd64"][~use].any() and np.abs(refs["fwd64"][use]).reshape(int(use.sum()), -1).max(1).min() > 0
    every = SC.align_refs("all")["bwd64"][0][:, :SC.AL_VALID_C]
    assert np.abs(every - refs["bwd64"][0]).max() > 100 * bound      # the counts take RoIs away that weigh


# ------------------------------------------------------------------------------------------------------------------- 2. RoIAlign sizes
@pytest.mark.parametrize("P,sampling,rows", [(32, 0, range(9)), (32, 2, (0, 3, 5)), (2, 9, range(9)), (7, 9, range(9)), (2, 64, (1, 3, 5, 6)), (7, 64, (3,))])
def test_mask_ref_against_the_naive_loop_at_the_caps(P, sampling, rows):
    """out_size 32 and the fixed grids 9 and 64: mask_ref against mmcv's loop written out one sample at a time (tests/test_mask_host.py)"""
    feats = SC.size_feats()
    rois, lv = SC.SZ_ROIS[list(rows)], SC.SZ_LEVELS[list(rows)]
    got, _ = MR.roi_align(feats, rois, SC.AL_STRIDES, P, sampling, True, SC.AL_FINEST, levels=lv)
    for r, roi in enumerate(rois):
        want = naive_roi_align(feats[lv[r]][int(roi[0])].astype(F64), roi[1:], 1.0 / SC.AL_STRIDES[lv[r]], P, sampling, True)
        assert float(np.abs(got[r] - want).max()) < 1e-12 * max(1.0, float(np.abs(want).max())), r


def test_size_cases_reach_what_they_are_for():
    assert sorted(SC.SZ_OUT_CASES) == sorted((P, s) for P in (1, 2, 31, 32) for s in (0, 2))
    assert sorted(SC.SZ_GRID_CASES) == sorted((P, s) for P in (2, 7) for s in (8, 9, 64)) and ops.ROI_ALIGN_MAX_OUT == 32 and ops.ROI_ALIGN_MAX_SAMPLING == 64
    grids = [MR.axis(r[1], r[3], 1.0 / SC.AL_STRIDES[l], 1, 0, True, F64)[2] for r, l in zip(SC.SZ_ROIS, SC.SZ_LEVELS)]
    assert max(grids) == 9 and 0 in grids      # out_size 1: an adaptive grid beyond the dense walk of 8; the zero-width box samples nothing
    n = len(SC.AL_SIZES)
    clamped = np.clip(SC.SZ_BAD_LEVELS, 0, n - 1)
    assert SC.SZ_BAD_LEVELS.min() < 0 and SC.SZ_BAD_LEVELS.max() == n + 3 and (clamped != SC.SZ_BAD_LEVELS).sum() == 3
    feats, d = SC.size_feats(), SC.size_dout(7)
    a = SC.size_refs(SC.SZ_ROIS, SC.SZ_BAD_LEVELS, 7, 2, d)
    b = SC.size_refs(SC.SZ_ROIS, clamped, 7, 2, d)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])), "the restatement clamps as the kernels do"
    assert np.abs(a[0] - SC.size_refs(SC.SZ_ROIS, SC.SZ_LEVELS, 7, 2, d)[0]).max() > 0.1, "the clamped levels are not the plain ones"
    bad = SC.bad_image_rois()
    gone = sorted(SC.SZ_BAD_IMAGES)
    assert sorted(np.float32(v) for v in SC.SZ_BAD_IMAGES.values() if v == v) == [-1.0, 2.0] and np.isnan(bad[7, 0]) and len(gone) == 3
    f64, _, g64, _ = SC.size_refs(bad, SC.SZ_LEVELS, 7, 2, d)
    keep = np.ones(len(bad), bool)
    keep[gone] = False
    assert not f64[gone].any() and np.abs(f64[keep]).reshape(int(keep.sum()), -1).max(1).min() > 0
    shapes = [f.shape for f in feats]
    rest = MR.roi_align_bwd(d[keep], shapes, bad[keep], SC.AL_STRIDES, 7, 2, True, SC.AL_FINEST, levels=SC.SZ_LEVELS[keep])
    assert all(np.array_equal(x, y) for x, y in zip(g64, rest)), "a RoI that names no image has no gradient"
    with_them = SC.size_refs(SC.SZ_ROIS, SC.SZ_LEVELS, 7, 2, d)[2]
    assert max(np.abs(x - y).max() for x, y in zip(g64, with_them)) > 0.1, "... and would have one on a valid image"


def test_wrappers_refuse_sizes_beyond_the_caps_before_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ops, "lib", boom)
    rois = torch.zeros(1, 5)
    for kw in (dict(out_size=33), dict(sampling_ratio=65), dict(out_size=0), dict(sampling_ratio=-1)):
        with pytest.raises(ValueError):
            ops.roi_align_fwd([], [(8, 8)], [0.25], 4, 1, rois, **kw)
        with pytest.raises(ValueError):
            ops.roi_align_bwd(torch.zeros(1, 4, 4), [], [(8, 8)], [0.25], 4, 1, rois, **kw)


# ------------------------------------------------------------------------------------------------------------------- 3. the mask loss
@pytest.mark.parametrize("M", SC.ML_SIZES)
def test_mask_size_seeds_keep_the_averages_off_the_threshold(M):
    c = SC.size_case(M)
    assert SC.avg_margin(c, c["n_pos"], M) > MC.MARGIN and SC.size_seed(M) == SC.ML_SEEDS[M]
    assert [m * m for m in SC.ML_SIZES] == [1, 4, 256, 289]      # far below the 256 threads, exactly one trip, one past it
    z = SC.loss_logits(len(c["boxes"]), MC.K, M, 40 + M)
    use, r64, r32 = SC.slot_refs(c, z, c["n_pos"], M)
    assert np.array_equal(r64["targets"], r32["targets"]) and r64["targets"][use].any() and not r64["targets"][use].all()


def test_slot_case_has_losses_on_the_second_trip():
    c = SC.slots_case()
    assert SC.slots_condition(c) and SC.SL_B * SC.SL_S == 99 and max(SC.SL_NPOS) <= 4 and c["sample_gt"].shape == (3, 33)
    use, r64, r32 = SC.slot_refs(c, c["logits"], c["n_pos"], MC.M)
    assert use[66:66 + SC.SL_NPOS[2]].all() and not use[66 + SC.SL_NPOS[2]:].any()
    bound, _ = SC.bound_of(r64["loss"], r32["loss"])
    share = r64["slot"] / (float(c["n_pos"].sum()) * MC.M * MC.M) * MC.LOSS_WEIGHT      # what a slot adds to the loss
    assert share[64:].max() > 100 * bound and (share[66:66 + SC.SL_NPOS[2]] > 100 * bound).all() and not share[:64][~use[:64]].any()
    assert np.array_equal(r64["targets"], r32["targets"])


def test_clamp_case_uses_every_slot_of_image_0():
    c = SC.clamp_case()
    assert SC.CLAMP_GIVEN == (MC.S + 5, -3) and SC.CLAMP_MEANT == (MC.S, 0)
    assert (c["sample_gt"][0] >= 0).all() and c["n_pos"][0] < MC.S and c["n_pos"][1] > 0      # the clamp adds a slot to image 0 and takes image 1's away
    assert SC.avg_margin(c, SC.CLAMP_MEANT, MC.M) > MC.MARGIN
    z = SC.loss_logits(len(c["boxes"]), MC.K, MC.M, 17)
    a, b = SC.slot_refs(c, z, SC.CLAMP_MEANT, MC.M)[1], SC.slot_refs(c, z, c["n_pos"], MC.M)[1]
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) > 1e-3 and a["slot"][MC.S - 1] > 0 and not a["slot"][MC.S:].any()


# ------------------------------------------------------------------------------------------------------------------- 4. the paste
def test_paste_case_has_its_nan_column():
    logits, labels, boxes, h, w = SC.paste_case()
    v64, m64 = MR.paste(logits, labels, boxes, h, w, MC.THR)
    v32, _ = MR.paste(logits, labels, boxes, h, w, MC.THR, ft=F32)
    nan = np.zeros(v64.shape, bool)
    nan[SC.PASTE_NAN_ROW, :, int(SC.PASTE_NAN_X)] = True
    assert np.array_equal(np.isnan(v64), nan) and np.array_equal(np.isnan(v32), nan) and nan.sum() == h
    assert not m64[nan].any() and not MR.paste(logits, labels, boxes, h, w, 0.0)[1][nan].any() and not MR.paste(logits, labels, boxes, h, w, -1.0)[1][nan].any()
    rest = v64[SC.PASTE_NAN_ROW][:, [c for c in range(w) if c != int(SC.PASTE_NAN_X)]]
    assert rest[10:28].min() > 0 and np.abs(rest - rest[:, :1]).max() == 0      # +-inf maps to 0: every other column samples the mask's centre column


# ------------------------------------------------------------------------------------------------------------------- 5. the box half
@pytest.mark.parametrize("S", SC.RL_S)
def test_rpn_loss_cases(S):
    c = SC.rpn_loss_case(S)
    assert SC.rpn_loss_condition(c) and sum(h * w * HC.A for h, w in HC.SIZES) == 1023 and c["samples"].shape == (HC.BATCH, S)
    n_pos, n_neg = c["n_pos"], c["n_neg"]
    assert n_pos[0] + n_neg[0] < S and n_pos[1] + n_neg[1] == S and n_pos[0] == S // 4 and -(-S // SC.RL_CHUNK) == {256: 1, 257: 2, 520: 3}[S]
    r64, r32 = SC.rpn_loss_refs(c)
    assert min(float(t.min()) for t in SC.rpn_l1_terms(c, r64)) > HC.THR_GAP
    assert all(np.array_equal(np.sign(a), np.sign(b)) for a, b in zip(r64[3], r32[3])) and (r64[0] > 0).all() and (r64[1] > 0).any()
    if S == 520:      # every chunk of image 1 holds a positive that weighs in loss_bbox
        bound, _ = SC.bound_of(r64[1], r32[1])
        assert n_pos[1] > 2 * SC.RL_CHUNK and min(SC.rpn_chunk_terms(c, r64)) > 100 * bound
    else:             # the slot past the first chunk (S = 257) is in use in image 1
        assert n_pos[1] == S // 4


@pytest.mark.parametrize("B,S,K", list(SC.RS_CASES))
def test_roi_loss_cases(B, S, K):
    case = SC.roi_loss_case(B, S, K)
    cls, reg, s = case
    assert SC.roi_loss_condition(case) and -(-B * S // 4) > 64      # more partial rows than the sum has lanes
    r64, r32 = SC.roi_loss_refs(cls, reg, K, s, "encoded")
    pos = np.nonzero((r64["labels"] >= 0) & (r64["labels"] < K))[0]
    assert pos.max() >= 256 and np.array_equal(r64["labels"], r32["labels"])      # a positive whose partial row is >= 64
    bound, _ = SC.bound_of(np.asarray(r64["loss_bbox"]).reshape(1), np.asarray(r32["loss_bbox"]).reshape(1))
    late = pos[pos >= 256]
    term = np.abs(np.stack([reg[q, 4 * r64["labels"][q]:4 * r64["labels"][q] + 4] for q in late]).astype(F64) - r64["targets"][late]).sum(1)
    assert (term / float((s["n_pos"] + s["n_neg"]).sum())).max() > 100 * bound


def test_proposal_case_spans_workgroups():
    cls, reg, _ = HC.planted()
    keep, counts = SC.proposal_keep(cls)
    T = sum(counts)
    assert counts == [100, 100, 48, 12, 3] and T == 263 and HC.BATCH * T == 526 and -(-HC.BATCH * T // 256) == 3
    starts = np.cumsum([0] + counts[:-1])
    assert T % 256 and all((b * T + s) % 256 for b in range(HC.BATCH) for s in starts[1:])      # no boundary falls on a workgroup's edge
    for min_size in SC.PROP_MIN_SIZES:
        assert SC.proposal_size_condition(cls, reg, keep, min_size)
    flags = []
    for (s64, b64, i64), (s32, b32, i32) in SC.proposal_refs(cls, reg, keep):
        assert np.array_equal(i64, i32) and i64.tolist() == sum(([l] * n for l, n in enumerate(counts)), [])
        for min_size in SC.PROP_MIN_SIZES:
            f = [((b[:, 2] - b[:, 0]) > min_size) & ((b[:, 3] - b[:, 1]) > min_size) for b in (b64, b32)]
            assert np.array_equal(f[0], f[1])
            flags.append(f[0])
    assert not all(f.all() for f in flags[1::2]) and any(f.any() for f in flags[1::2])      # min_size 6 drops some and keeps some
