"""CPU: the oriented RPN without a device.
  * tests/rpn_ref.py against fixture f22 (the reference's own head run in float64, tests/golden/make_oriented_rpn.py): targets, losses, gradients,
    kept proposals -- and against itself: decode(encode(prior, box)) gives the box back, the numbers of the issue (4092 anchors, 1884 inside);
  * the conditions of tests/rpn_cases.py hold for the seeds it names, and those are the first seeds that meet them;
  * registry names, state-dict keys, every refusal; the new entry points reject NULL arguments before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_cases as BC
import rpn_cases as RC
import rpn_ref as R

CASES = list(RC.SHAPES)


@pytest.fixture(scope="module")
def f22(golden):
    return golden("f22_oriented_rpn.npz")


def sampled(f22, name):
    """per image the flat anchor indices of the recorded samples and the gt rows of the positives"""
    inside = np.nonzero(RC.anchors(name)[1])[0]
    q = [("%s.image%d." % (name, b)) for b in range(RC.BATCH)]
    return [inside[f22[p + "pos_inds"]] for p in q], [f22[p + "pos_gt"] for p in q], [inside[f22[p + "neg_inds"]] for p in q]


# ------------------------------------------------------------------------------------------------------------------- rpn_ref
def test_anchor_counts():
    priors, inside, sizes = RC.anchors("sq128")
    assert sizes == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)] and len(priors) == 4092 and int(inside.sum()) == 1884
    assert RC.anchors("pad160")[2] == [(32, 40), (16, 20), (8, 10), (4, 5), (2, 3)]
    base = R.base_anchors(4, RC.SCALES, RC.RATIOS)
    assert base.dtype == np.float32 and np.allclose(base[1], [-16, -16, 16, 16]) and np.allclose(base[0], [-22.627417, -11.313708, 22.627417, 11.313708])
    # the pad columns of the 96 x 160 image: rows 24 .. 32 of level 0 are inside the padding, their anchors are not valid for a pad_shape of 96 rows
    p = R.grid_priors(base, 32, 40, (4, 4))
    assert int(R.inside_flags(p, 3, 32, 40, (4, 4), (96, 160), (96, 160), -1).sum()) == 24 * 40 * 3


def test_decode_inverts_encode():
    """a rotated rectangle's midpoint offsets decode to the rectangle itself, w >= h and theta in [-pi/2, pi/2): the closed form is the coder's inverse"""
    rng = np.random.default_rng(1)
    n = 400
    p = np.stack([rng.uniform(0, 80, n), rng.uniform(0, 80, n)], 1)
    p = np.concatenate([p, p + rng.uniform(16, 64, (n, 2))], 1)
    g = np.stack([rng.uniform(20, 100, n), rng.uniform(20, 100, n), rng.uniform(20, 60, n), rng.uniform(4, 19, n), rng.uniform(-np.pi / 2, np.pi / 2, n)], 1)
    X, Y = R.corners(g)      # within 0.1 px of axis-aligned the coder takes the farther of two corners: those boxes do not come back, by design
    clear = (np.sort(np.abs(Y - Y.min(1, keepdims=True)), 1)[:, 1] > 0.1) & (np.sort(np.abs(X - X.max(1, keepdims=True)), 1)[:, 1] > 0.1)
    p, g = p[clear], g[clear]
    assert clear.sum() > 350
    back = R.decode(p, R.encode(p, g, RC.MEANS, RC.STDS), RC.MEANS, RC.STDS)
    assert np.abs(back - g).max() < 1e-9
    g2 = g.copy()      # the same box named with its sides swapped
    g2[:, 2], g2[:, 3], g2[:, 4] = g[:, 3], g[:, 2], np.where(g[:, 4] < 0, g[:, 4] + np.pi / 2, g[:, 4] - np.pi / 2)
    assert np.abs(R.decode(p, R.encode(p, g2, RC.MEANS, RC.STDS), RC.MEANS, RC.STDS) - g).max() < 1e-9


def test_decode_clamps_and_collapse():
    p = np.array([[10.0, 20.0, 42.0, 52.0]] * 4)
    d = np.array([[0, 0, 9, -9, 0.1, 0.2], [0, 0, 0, 0, 1.0, -1.0], [0, 0, 0, 0, -3.0, 3.0], [0, 0, 0, 0, 1.0, 1.0]], np.float64)
    for dtype in (np.float64, np.float32):
        out = R.decode(p, d, RC.MEANS, RC.STDS, dtype)
        assert np.isfinite(out).all()
        # the size clamp: exp(+-|log(16 / 1000)|) of the prior's 32 x 32
        c0, c1 = np.array([0.05 * 2000.0, -0.256]), np.array([1000.0, 0.1 * 0.512])      # the vertices of the 2000 x 0.512 box before the rescaling
        assert abs(np.hypot(*(c1 - c0 * np.hypot(*c1) / np.hypot(*c0))) - out[0, 3]) < 1e-4
        assert out[1, 3] == 0 and out[2, 3] == 0 and out[1, 2] > 0 and out[2, 2] > 0      # da = +-0.5, db = -+0.5: a segment
        assert abs(out[3, 2] - 32) < 1e-4 and abs(out[3, 3] - 32) < 1e-4                  # da = db = 0.5: the prior's own square


@pytest.mark.parametrize("name", CASES)
def test_ref_targets_and_loss_vs_f22(f22, name):
    cls, reg, gts = RC.case(name)
    priors, inside, sizes = RC.anchors(name)
    pos, pgt, neg = sampled(f22, name)
    for l in range(len(sizes)):
        assert np.array_equal(f22["%s.level%d.cls" % (name, l)], cls[l]) and np.array_equal(f22["%s.level%d.reg" % (name, l)], reg[l])
    assert int(f22[name + ".avg_factor"]) == sum(len(p) + len(n) for p, n in zip(pos, neg)) == RC.BATCH * RC.NUM
    lc, lb, dcls, dreg = R.loss(cls, reg, sizes, RC.A, priors, gts, pos, pgt, neg, RC.MEANS, RC.STDS, RC.BETA)
    assert np.abs(lc - f22[name + ".loss_cls"]).max() < 1e-12 and np.abs(lb - f22[name + ".loss_bbox"]).max() < 1e-12
    firsts = np.cumsum([0] + [h * w * RC.A for h, w in sizes])
    for l in range(len(sizes)):
        q = "%s.level%d." % (name, l)
        assert np.abs(dcls[l] - f22[q + "dcls"]).max() < 1e-14 and np.abs(dreg[l] - f22[q + "dreg"]).max() < 1e-14
        # the reference's per-level targets: labels 0 on positives and 1 (background) elsewhere, weights 1 on the samples, the encoded boxes
        n = firsts[l + 1] - firsts[l]
        for b in range(RC.BATCH):
            lab, lw = np.ones(n, np.int8), np.zeros(n, np.int8)
            bt, bw = np.zeros((n, 6)), np.zeros((n, 6), np.int8)
            pl = (pos[b] >= firsts[l]) & (pos[b] < firsts[l + 1])
            nl = (neg[b] >= firsts[l]) & (neg[b] < firsts[l + 1])
            lab[pos[b][pl] - firsts[l]] = 0
            lw[pos[b][pl] - firsts[l]] = 1
            lw[neg[b][nl] - firsts[l]] = 1
            if pl.any():
                bt[pos[b][pl] - firsts[l]] = R.encode(priors[pos[b][pl]], gts[b].astype(np.float64)[pgt[b][pl]], RC.MEANS, RC.STDS)
                bw[pos[b][pl] - firsts[l]] = 1
            assert np.array_equal(f22[q + "labels"][b], lab) and np.array_equal(f22[q + "label_weights"][b], lw)
            assert np.array_equal(f22[q + "bbox_weights"][b], bw) and np.abs(f22[q + "bbox_targets"][b] - bt).max() < 1e-13


@pytest.mark.parametrize("name", CASES)
def test_ref_samples_follow_the_assignment(f22, name):
    """the recorded choice: positives among gt_inds > 0 with their gt, negatives among gt_inds == 0, the cap of num * pos_fraction in force"""
    gts = RC.case(name)[2]
    capped = False
    for b in range(RC.BATCH):
        q = "%s.image%d." % (name, b)
        gt_inds = RC.assign64(name, gts[b])[0]
        p, n = f22[q + "pos_inds"], f22[q + "neg_inds"]
        assert (gt_inds[p] > 0).all() and (gt_inds[n] == 0).all() and np.array_equal(gt_inds[p] - 1, f22[q + "pos_gt"])
        assert len(p) == min(int((gt_inds > 0).sum()), int(RC.NUM * RC.POS_FRACTION)) and len(n) == RC.NUM - len(p)
        capped = capped or int((gt_inds > 0).sum()) > len(p)
    assert capped


@pytest.mark.parametrize("tag,min_size", [("prop", 0), ("prop_min", RC.MIN_SIZE)])
@pytest.mark.parametrize("name", CASES)
def test_ref_proposals_vs_f22(f22, name, tag, min_size):
    cls, reg, _ = RC.case(name)
    priors, _, sizes = RC.anchors(name)
    for b in range(RC.BATCH):
        keep, rb, sc = R.proposals([m[b] for m in cls], [m[b] for m in reg], priors, sizes, RC.A, RC.MEANS, RC.STDS, RC.PROPOSAL["nms_pre"],
                                   RC.PROPOSAL["max_per_img"], RC.PROPOSAL["nms"]["iou_threshold"], min_size)
        q = "%s.%s.image%d." % (name, tag, b)
        assert np.array_equal(keep, f22[q + "keep"]) and np.abs(rb - f22[q + "bboxes"]).max() < 1e-12 and np.abs(sc - f22[q + "scores"]).max() < 1e-15
        assert (np.diff(sc) < 0).all() and (rb[:, 2] > min_size).all() and (rb[:, 3] > min_size).all()
    # the size filter bites: the two runs differ
    assert not np.array_equal(f22["%s.prop.image0.keep" % name], f22["%s.prop_min.image0.keep" % name])


# ------------------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", CASES)
def test_case_conditions(name):
    case = RC.case(name)
    assert RC.condition(name, case)
    assert BC.first_seed(lambda s: RC._try(name, s), lambda c: RC.condition(name, c)) == RC.SEEDS[name]
    gts = case[2]
    assert [len(g) for g in gts] == list(RC.SHAPES[name][2])
    if name == "sq128":
        gt_inds, mx, _ = RC.assign64(name, gts[0])
        pos = gt_inds > 0
        assert (pos & (mx >= 0.7)).any() and (pos & (mx < 0.7)).any() and int(pos.sum()) > RC.NUM * RC.POS_FRACTION
    else:
        assert (RC.assign64(name, gts[1])[0] == 0).all()      # no gt: every anchor inside the image is background


# ------------------------------------------------------------------------------------------------------------------- the Python surface
TRAIN_CFG = dict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="mmrotate.RBbox2HBboxOverlaps2D"), **RC.ASSIGNER),
                 sampler=dict(type="RandomSampler", num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False), allowed_border=0, pos_weight=-1,
                 debug=False)
HEAD_CFG = dict(type="MTP_RD_OrientedRPNHead", in_channels=256, feat_channels=256,
                anchor_generator=dict(type="mmdet.AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64], use_box_type=True),
                bbox_coder=dict(type="MidpointOffsetCoder", angle_version="le90", target_means=[0.0] * 6, target_stds=[1.0, 1.0, 1.0, 1.0, 0.5, 0.5]),
                loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=0.1111111111111111, loss_weight=1.0))


def test_registry_names_and_state_dict():
    from mtp_amd import MODELS, TASK_UTILS
    from mtp_amd.dense_heads import OrientedRPNHead
    from mtp_amd.task_modules import AnchorGenerator, MidpointOffsetCoder, RandomSampler
    assert MODELS.get("OrientedRPNHead") is OrientedRPNHead and MODELS.get("MTP_RD_OrientedRPNHead") is OrientedRPNHead
    assert TASK_UTILS.get("AnchorGenerator") is AnchorGenerator and TASK_UTILS.get("mmdet.AnchorGenerator") is AnchorGenerator
    assert TASK_UTILS.get("RandomSampler") is RandomSampler and TASK_UTILS.get("MTP_RD_RandomSampler") is RandomSampler
    assert TASK_UTILS.get("MidpointOffsetCoder") is MidpointOffsetCoder and MidpointOffsetCoder.encode_size == 6
    head = MODELS.build(dict(HEAD_CFG, train_cfg=TRAIN_CFG, test_cfg=RC.PROPOSAL))      # the reference's configuration, oriented_rcnn.py:20-40, 77-99
    assert list(head.state_dict()) == ["rpn_conv.weight", "rpn_conv.bias", "rpn_cls.weight", "rpn_cls.bias", "rpn_reg.weight", "rpn_reg.bias"]
    assert tuple(head.rpn_conv.weight.shape) == (256, 256, 3, 3) and tuple(head.rpn_cls.weight.shape) == (3, 256, 1, 1)
    assert tuple(head.rpn_reg.weight.shape) == (18, 256, 1, 1)
    gen = head.prior_generator
    assert gen.num_levels == 5 and gen.num_base_priors == [3] * 5 and gen.strides == [(s, s) for s in RC.STRIDES]
    for b, s in zip(gen.base_anchors, RC.STRIDES):
        assert torch.equal(b, torch.from_numpy(R.base_anchors(s, RC.SCALES, RC.RATIOS)))
    assert head.sampler.num == 256 and head.assigner.pos_iou_thr == 0.7 and head.beta == 0.1111111111111111


def test_refusals():
    from mtp_amd import MODELS
    from mtp_amd.task_modules import AnchorGenerator, AssignResult, MidpointOffsetCoder, RandomSampler
    gen = dict(strides=[4, 8], ratios=[1.0], scales=[8])
    for bad in (dict(octave_base_scale=4, scales_per_octave=3), dict(centers=[(0, 0), (0, 0)]), dict(center_offset=0.5)):
        with pytest.raises(NotImplementedError):
            AnchorGenerator(**dict(gen, **bad))
    with pytest.raises(NotImplementedError):
        RandomSampler(num=256, pos_fraction=0.5, neg_pos_ub=3, add_gt_as_proposals=False)
    with pytest.raises(NotImplementedError):
        RandomSampler(num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=True)
    with pytest.raises(NotImplementedError):
        RandomSampler(num=256, pos_fraction=0.5)      # the reference's default is add_gt_as_proposals=True
    with pytest.raises(NotImplementedError):
        MidpointOffsetCoder(angle_version="oc")
    for bad in (dict(num_convs=2), dict(loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False)), dict(reg_decoded_bbox=True),
                dict(train_cfg=dict(TRAIN_CFG, pos_weight=2.0)), dict(loss_bbox=dict(type="L1Loss"))):
        with pytest.raises(NotImplementedError):
            MODELS.build(dict(HEAD_CFG, **bad))
    with pytest.raises(ValueError):
        MODELS.build(dict(HEAD_CFG, precision="fp16"))
    with pytest.raises(RuntimeError):      # no CPU fallback
        MidpointOffsetCoder().encode(torch.zeros(2, 4), torch.zeros(2, 5))
    with pytest.raises(ValueError):
        RandomSampler(4, 0.5, add_gt_as_proposals=False).sample(AssignResult(1, torch.zeros(8, dtype=torch.int64), None, None), pos_inds=[0, 1, 2], neg_inds=[3, 4])


def test_sampler_on_the_host():
    """the sampler is torch plumbing: its rules hold on any device"""
    from mtp_amd.task_modules import AssignResult, RandomSampler
    gt_inds = torch.tensor([2, 0, 0, -1, 1, 1, 0, 2, 0, 0, -1, 2, 0, 0, 1], dtype=torch.int64)
    s = RandomSampler(8, 0.25, add_gt_as_proposals=False)
    g = torch.Generator().manual_seed(3)
    a = s.sample(AssignResult(2, gt_inds, None, None), generator=g)
    assert int(a.n_pos) == 2 and int(a.n_neg) == 6 and (gt_inds[a.pos_inds] > 0).all() and (gt_inds[a.neg_inds] == 0).all()
    assert len(set(a.inds.tolist())) == 8 and torch.equal(a.gt_inds[:2], gt_inds[a.pos_inds] - 1) and (a.gt_inds[2:] == -1).all()
    b = s.sample(AssignResult(2, gt_inds, None, None), generator=torch.Generator().manual_seed(3))
    assert torch.equal(a.inds, b.inds)
    few = RandomSampler(16, 0.5, add_gt_as_proposals=False).sample(AssignResult(2, gt_inds, None, None))      # fewer candidates than asked for
    assert int(few.n_pos) == 6 and int(few.n_neg) == 7 and sorted(few.pos_inds.tolist()) == [0, 4, 5, 7, 11, 14]
    none = s.sample(AssignResult(0, torch.zeros(5, dtype=torch.int64), None, None))
    assert int(none.n_pos) == 0 and int(none.n_neg) == 5
    ex = s.sample(AssignResult(2, gt_inds, None, None), pos_inds=[4, 0], neg_inds=[1, 2, 6])
    assert ex.inds[:5].tolist() == [4, 0, 1, 2, 6] and ex.gt_inds[:2].tolist() == [0, 1] and int(ex.n_pos) == 2 and int(ex.n_neg) == 3


def test_new_entry_points_reject_null_arguments():
    from mtp_amd import _lib
    lib = _lib.load()
    six = (C.c_float * 6)(1, 1, 1, 1, 1, 1)
    lv = (_lib.RpnLevel * 1)()
    P = 1 << 20
    assert lib.mtp_rpn_anchors(None, 3, 4, 4, 4, 4, 16, 16, 16, 16, 0.0, P, P, None) == -1
    assert lib.mtp_rpn_anchors(P, 3, 0, 4, 4, 4, 16, 16, 16, 16, 0.0, P, P, None) == -1
    assert lib.mtp_rpn_anchors(P, 3, 4, 4, 0, 4, 16, 16, 16, 16, 0.0, P, P, None) == -1
    assert lib.mtp_rpn_encode(None, P, six, six, 4, P, None) == -1 and lib.mtp_rpn_encode(P, P, None, six, 4, P, None) == -1
    assert lib.mtp_rpn_decode(P, P, six, six, 0, P, None) == -1 and lib.mtp_rpn_decode(P, P, six, (C.c_float * 6)(1, 1, 1, 1, 0, 1), 4, P, None) == -1
    assert lib.mtp_rpn_loss_workspace_bytes(0, 16) == -1 and lib.mtp_rpn_loss_workspace_bytes(2, 300) == 2 * 2 * 2 * _lib.RPN_MAX_LEVELS * 4
    # a level without maps, levels that do not add up to the priors, a sample list without counts
    assert lib.mtp_rpn_loss(lv, 1, 3, P, 48, P, 1, P, P, P, P, 1, 16, six, six, 0.1, 1.0, 1.0, P, P, P, 1 << 10, None) == -1
    lv[0].cls, lv[0].reg, lv[0].H, lv[0].W = P, P, 4, 4
    assert lib.mtp_rpn_loss(lv, 1, 3, P, 47, P, 1, P, P, P, P, 1, 16, six, six, 0.1, 1.0, 1.0, P, P, P, 1 << 10, None) == -1
    assert lib.mtp_rpn_loss(lv, 1, 3, P, 48, P, 1, P, P, None, P, 1, 16, six, six, 0.1, 1.0, 1.0, P, P, P, 1 << 10, None) == -1
    assert lib.mtp_rpn_loss(lv, 1, 3, P, 48, P, 1, P, P, P, P, 1, 16, six, six, 0.0, 1.0, 1.0, P, P, P, 1 << 10, None) == -1       # beta
    assert lib.mtp_rpn_loss(lv, 1, 3, P, 48, P, 1, P, P, P, P, 1, 16, six, six, 0.1, 1.0, 1.0, P, P, P, 8, None) == -1             # workspace
    assert lib.mtp_rpn_loss(lv, 9, 3, P, 48, P, 1, P, P, P, P, 1, 16, six, six, 0.1, 1.0, 1.0, P, P, P, 1 << 10, None) == -1       # levels
    lv[0].keep_count = 49      # more kept anchors than the level has
    assert lib.mtp_rpn_proposals(lv, 1, 3, P, 48, P, 1, six, six, 0.0, P, P, P, P, P, None) == -1
    lv[0].keep_count = 0       # nothing kept at all
    assert lib.mtp_rpn_proposals(lv, 1, 3, P, 48, P, 1, six, six, 0.0, P, P, P, P, P, None) == -1
    lv[0].keep_count = 8
    assert lib.mtp_rpn_proposals(lv, 1, 3, P, 48, None, 1, six, six, 0.0, P, P, P, P, P, None) == -1
