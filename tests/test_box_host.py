"""CPU: the float64 reference of the box operators (tests/box_ref.py) against closed forms and against the reference's own assigner runs (fixture f21);
the conditions every GPU test input must meet (tests/box_cases.py), from the float64 reference alone; the Python surface of mtp_amd.ops_box and
mtp_amd.task_modules where it needs no device: registry names, empty inputs, refusals, assign_wrt_overlaps in torch."""
import math

import numpy as np
import pytest
import torch

import box_cases as C
import box_ref as R


# ------------------------------------------------------------------------------------------------------------------- box_ref, analytic
def test_rotated_iou_closed_forms():
    assert abs(R.box_iou_rotated([[0, 0, 1, 1, 0]], [[0, 0, 1, 1, math.pi / 4]])[0, 0] - 1 / math.sqrt(2)) < 1e-12
    b = [30, 40, 20, 8, 0.7]
    same = R.box_iou_rotated([b, b, b], [b, [30, 40, 20, 8, 0.7 + math.pi], [30, 40, 8, 20, 0.7 + math.pi / 2]], aligned=True)
    assert np.abs(same - 1).max() < 1e-12
    assert abs(R.box_iou_rotated([[5, 5, 2, 2, 0.3]], [[5, 5, 10, 10, 0.3]])[0, 0] - 0.04) < 1e-12
    assert abs(R.box_iou_rotated([[5, 5, 2, 2, 0.3]], [[5, 5, 10, 10, 0.3]], mode="iof")[0, 0] - 1) < 1e-12
    assert R.box_iou_rotated([[5, 5, 2, 2, 0.3]], [[50, 5, 10, 10, 0.3]])[0, 0] == 0.0
    assert R._rot_pairs(np.array([[5, 5, 2, 2, 0.3]]), np.array([[50, 5, 10, 10, 1.3]]), "iou", R.F64)[0] == 0.0      # the clipping itself, no prefilter
    t, d = 0.3, np.arange(10)
    row = np.stack([100 + d * math.cos(t), 100 + d * math.sin(t), np.full(10, 10.0), np.full(10, 10.0), np.full(10, t)], 1)
    assert np.abs(R.box_iou_rotated(row[:1], row)[0] - (10 - d) / (10 + d)).max() < 1e-12
    assert R.box_iou_rotated([[1, 1, 0, 5, 0]], [[1, 1, 4, 5, 0]])[0, 0] == 0.0                                       # an area below 1e-14


def test_rotated_iou_at_angle_zero_is_the_aligned_iou_and_the_prefilter_changes_nothing():
    rng = np.random.default_rng(0)
    h1, h2 = C.rand_boxes(40, rng, False), C.rand_boxes(50, rng, False)
    r1, r2 = C.hbox_to_rbox(h1, np.zeros(40)), C.hbox_to_rbox(h2, np.zeros(50))
    assert np.abs(R.box_iou_rotated(r1, r2) - R.bbox_overlaps(h1, h2)).max() < 1e-12
    a, b = C.rand_boxes(40, rng, True), C.rand_boxes(50, rng, True)
    full = R._rot_pairs(np.repeat(a.astype(R.F64), 50, 0), np.tile(b.astype(R.F64), (40, 1)), "iou", R.F64).reshape(40, 50)
    assert np.array_equal(R.box_iou_rotated(a, b), full) and (full > 0).any() and (full == 0).any()
    assert np.abs(R.box_iou_rotated(a, b, dtype=R.F32) - full).max() < 1e-5


def test_aligned_iou_and_circumscribed_box():
    assert R.bbox_overlaps([[0, 0, 10, 10]], [[5, 0, 15, 10]])[0, 0] == 50 / 150 and R.bbox_overlaps([[0, 0, 10, 10]], [[5, 0, 15, 10]], "iof")[0, 0] == 0.5
    assert R.bbox_overlaps([[0, 0, 0, 0]], [[0, 0, 0, 0]])[0, 0] == 0.0 and R.bbox_overlaps([[0, 0, 10, 10]], [[10, 0, 20, 10]])[0, 0] == 0.0
    h = R.rbox2hbox([[10, 20, 8, 4, math.pi / 2], [10, 20, 2, 2, math.pi / 4]])
    assert np.abs(h - [[8, 16, 12, 24], [10 - math.sqrt(2), 20 - math.sqrt(2), 10 + math.sqrt(2), 20 + math.sqrt(2)]]).max() < 1e-12


def test_greedy_nms_chains_groups_and_stable_order():
    b = np.array([[0, 0, 10, 10], [1, 0, 11, 10], [2, 0, 12, 10], [100, 0, 110, 10]], float)      # A removes B, so B does not remove C
    assert R.nms(b, [0.9, 0.8, 0.7, 0.6], 0.7).tolist() == [0, 2, 3]
    assert R.nms(b, [0.9, 0.8, 0.7, 0.6], 0.7, groups=[0, 1, 0, 0]).tolist() == [0, 1, 2, 3]
    assert R.nms(b, [0.5, 0.5, 0.5, 0.9], 0.5).tolist() == [3, 0]


# ------------------------------------------------------------------------------------------------------------------- box_ref's assigner against f21
def test_box_ref_assigner_equals_the_reference_runs(golden):
    from make_box_ops import RUNS
    from mtp_amd import TASK_UTILS
    g = golden("f21_box_ops.npz")
    assert len(RUNS) == 6 and {c for c, _ in RUNS} == set(C.ASSIGN_CFGS) and {k for _, k in RUNS} == set(R.KINDS)
    for cfg, kind in RUNS:
        gts, priors, labels = g[kind + ".gts"], g[kind + ".priors"], g[kind + ".labels"]
        assert gts.dtype == priors.dtype == np.float32
        ov = R.overlaps(gts, priors, kind)
        assert C.assign_condition(ov), (cfg, kind)
        p = "%s.%s." % (cfg, kind)
        got = R.assign_wrt_overlaps(ov, labels, **C.ASSIGN_CFGS[cfg])
        for a, name in zip(got, ("gt_inds", "max_overlaps", "labels")):
            assert a.dtype == g[p + name].dtype and np.array_equal(a, g[p + name]), (cfg, kind, name)
        # the torch statement kept for callers that hold a matrix
        res = TASK_UTILS.build(dict(type="MTP_RD_MaxIoUAssigner", **C.ASSIGN_CFGS[cfg])).assign_wrt_overlaps(torch.from_numpy(ov), torch.from_numpy(labels))
        assert res.num_gts == len(gts) and np.array_equal(res.gt_inds.numpy(), got[0]) and np.array_equal(res.labels.numpy(), got[2])
        assert np.array_equal(res.max_overlaps.numpy(), got[1])
    assert len({int((g[p + "gt_inds"] > 0).sum()) for p in ("rpn.rbox2hbox.", "rcnn_off.rotated.", "rpn.box.", "rcnn_on.box.")}) > 1


# ------------------------------------------------------------------------------------------------------------------- the GPU tests' inputs
def test_nms_inputs_meet_their_condition_and_the_seeds_are_the_first():
    for rotated in (False, True):
        for n in C.NMS_SIZES[rotated]:
            boxes, scores, groups = C.nms_set(n, rotated)
            assert boxes.dtype == scores.dtype == np.float32 and C.nms_condition(boxes, scores, rotated)
            assert C.first_seed(lambda s: C._nms_try(n, s, rotated), lambda t: C.nms_condition(t[0], t[1], rotated)) == C.NMS_SEEDS[(rotated, n)]
        assert max(C.NMS_SIZES[rotated]) <= (65 if rotated else 129)
        # the chain set: its overlaps take only the values (10 - d) / (10 + d), none nearer than 0.011 to a threshold
        boxes, scores = C.chain_set(rotated)
        assert len(boxes) == 2049 and len(np.unique(scores)) == 2049
        iou = C.iou64(boxes, boxes, rotated)
        values = (10.0 - np.arange(11)) / (10.0 + np.arange(11))
        assert np.abs(iou[:, :, None] - values[None, None]).min(2).max() < 1e-4      # (centres rounded to float32 at up to 3300 px: 2.4e-4 px)
        m = C.chain_margins(rotated)
        assert all(abs(m[t] - w) < 1e-3 for t, w in zip(C.NMS_THRS[rotated], ((0.011 if rotated else 0.033), 0.038, 0.033, 0.018)))
        assert C.clear_of(iou, C.NMS_THRS[rotated], 0.01)


def test_assignment_inputs_meet_their_condition_and_the_seeds_are_the_first():
    for kind in R.KINDS:
        for K, N in C.ASSIGN_SIZES:
            gts, priors, labels, ov = C.assign_set(K, N, kind)
            assert gts.dtype == priors.dtype == np.float32 and ov.shape == (K, N) and C.assign_condition(ov)
            if (kind, K, N) != ("rotated", 65, 1000):      # seed 30: the search clips 31 x 65 000 rotated pairs, 8 s; `python tests/box_cases.py` runs it
                assert C.first_seed(lambda s: C._assign_try(K, N, s, kind), lambda t: C.assign_condition(R.overlaps(t[0], t[1], kind))) == C.ASSIGN_SEEDS[(kind, K, N)]
        # more gts than one LDS tile of the kernels, an exact duplicate pair across the boundary (the condition's one exemption)
        gts, priors, labels, ov = C.big_set(kind)
        assert ov.shape == (C.BIG_K, C.BIG_N) and C.BIG_K > C.TILE == 256 and C.big_condition(ov) and C.BIG_SEEDS[kind] == 0
    for rotated in (False, True):
        boxes, scores = C.chain_set(rotated, C.CHAIN_N_WIDE)
        assert len(boxes) == 4225 > 64 * 64 and len(np.unique(scores)) == 4225 and C.clear_of(C.iou64(boxes, boxes, rotated), C.NMS_THRS[rotated], 0.01)
    # the condition sees what it is there for
    assert not C.assign_condition(np.array([[0.7 + 5e-5, 0.2]])) and not C.assign_condition(np.array([[0.6, 0.2], [0.6 + 5e-5, 0.1]]))
    assert not C.assign_condition(np.array([[0.6, 0.6, 0.1]])) and not C.assign_condition(np.array([[0.3 - 5e-5, 0.2]]))
    assert C.assign_condition(np.array([[0.6, 0.0], [0.2, 0.0], [0.0, 0.45]]))


# ------------------------------------------------------------------------------------------------------------------- surface
def test_registry_names_and_exports():
    import mtp_amd
    from mtp_amd import TASK_UTILS, task_modules
    for name in ("AssignResult", "BboxOverlaps2D", "RBboxOverlaps2D", "RBbox2HBboxOverlaps2D", "MaxIoUAssigner", "bbox_overlaps", "box_iou_rotated", "nms",
                 "nms_rotated", "batched_nms", "TASK_UTILS"):
        assert hasattr(mtp_amd, name), name
    assert TASK_UTILS.get("MaxIoUAssigner") is task_modules.MaxIoUAssigner and TASK_UTILS.get("MTP_RD_MaxIoUAssigner") is task_modules.MTP_RD_MaxIoUAssigner
    assert issubclass(task_modules.MTP_RD_MaxIoUAssigner, task_modules.MaxIoUAssigner)
    assert TASK_UTILS.get("MTP_RD_RBbox2HBboxOverlaps2D") is TASK_UTILS.get("RBbox2HBboxOverlaps2D") is task_modules.RBbox2HBboxOverlaps2D
    assert TASK_UTILS.get("BboxOverlaps2D") is task_modules.BboxOverlaps2D and TASK_UTILS.get("RBboxOverlaps2D") is task_modules.RBboxOverlaps2D
    # the dicts of oriented_rcnn.py:78-108 and mask_rcnn.py:72-99
    a = TASK_UTILS.build(dict(type="MTP_RD_MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1,
                              iou_calculator=dict(type="MTP_RD_RBbox2HBboxOverlaps2D")))
    assert a.iou_calculator.kind == "rbox2hbox" and a.gt_max_assign_all and a.gpu_assign_thr == -1
    a = TASK_UTILS.build(dict(type="MTP_RD_MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1,
                              iou_calculator=dict(type="mmrotate.RBboxOverlaps2D")))
    assert a.iou_calculator.kind == "rotated" and not a.match_low_quality
    a = TASK_UTILS.build(dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=(0.1, 0.3), min_pos_iou=0.3, gpu_assign_thr=100))
    assert a.iou_calculator.kind == "box" and a.neg_iou_thr == (0.1, 0.3)
    assert task_modules.MaxIoUAssigner(0.5, 0.5, iou_calculator=dict(type="mmdet.BboxOverlaps2D", scale=2.)).iou_calculator.scale == 2.
    assert "scale=1.0" in repr(task_modules.RBboxOverlaps2D())


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_gt_field_precedence_of_the_two_assigner_names():
    """MTP_RD_MaxIoUAssigner reads .rboxes / .rlabels first, as the reference does (max_iou_assigner.py:190-192); MaxIoUAssigner .bboxes / .labels.  Seen
    through the K = 0 path, which needs no device: the empty field decides"""
    from mtp_amd import MTP_RD_MaxIoUAssigner, MaxIoUAssigner
    lab0, lab2 = torch.zeros(0, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    both = Bag(bboxes=torch.zeros(0, 4), labels=lab0, rboxes=torch.ones(2, 4), rlabels=lab2)
    pri = Bag(priors=torch.zeros(0, 4))
    assert MaxIoUAssigner(0.5, 0.5).assign(pri, both).num_gts == 0 and MTP_RD_MaxIoUAssigner(0.5, 0.5).assign(pri, both).num_gts == 2
    only_h, only_r = Bag(bboxes=torch.ones(3, 4), labels=lab2), Bag(rboxes=torch.ones(2, 4), rlabels=lab2)
    assert MTP_RD_MaxIoUAssigner(0.5, 0.5).assign(pri, only_h).num_gts == 3 and MaxIoUAssigner(0.5, 0.5).assign(pri, only_r).num_gts == 2


def test_empty_inputs_on_cpu_tensors():
    from mtp_amd import MaxIoUAssigner, batched_nms, bbox_overlaps, box_iou_rotated, nms, nms_rotated
    z4, z5, z = torch.zeros(0, 4), torch.zeros(0, 5), torch.zeros(0)
    assert bbox_overlaps(z4, torch.ones(3, 4)).shape == (0, 3) and bbox_overlaps(torch.ones(3, 4), z4).shape == (3, 0)
    assert bbox_overlaps(z4, z4, is_aligned=True).shape == (0,) and bbox_overlaps(z4, z4).dtype == torch.float32
    assert box_iou_rotated(z5, torch.ones(2, 5)).shape == (0, 2) and box_iou_rotated(z5, z5, aligned=True).shape == (0,)
    dets, inds = nms(z4, z, 0.5)
    assert dets.shape == (0, 5) and inds.shape == (0,) and inds.dtype == torch.int64
    dets, inds = nms(torch.ones(3, 4), torch.zeros(3), 0.5, score_threshold=0.1)      # nothing passes the score threshold
    assert dets.shape == (0, 5) and inds.shape == (0,) and inds.dtype == torch.int64
    dets, inds = nms_rotated(z5, z, 0.1, labels=torch.zeros(0, dtype=torch.int64))
    assert dets.shape == (0, 6) and inds.shape == (0,) and inds.dtype == torch.int64
    for kind, zb in (("nms", z4), ("nms_rotated", z5)):
        dets, inds = batched_nms(zb, z, torch.zeros(0, dtype=torch.int64), dict(type=kind, iou_threshold=0.5, max_num=10, split_thr=100))
        assert dets.shape == (0, zb.shape[1] + 1) and inds.shape == (0,) and inds.dtype == torch.int64
    for calc, gz, pz in (("BboxOverlaps2D", z4, z4), ("RBbox2HBboxOverlaps2D", z5, z4), ("RBboxOverlaps2D", z5, z5)):
        a = MaxIoUAssigner(0.7, 0.3, iou_calculator=dict(type=calc))
        res = a.assign(Bag(priors=torch.ones(6, pz.shape[1])), Bag(bboxes=gz, labels=torch.zeros(0, dtype=torch.int64)))
        assert res.num_gts == 0 and res.gt_inds.tolist() == [0] * 6 and res.labels.tolist() == [-1] * 6 and res.max_overlaps.tolist() == [0.0] * 6
        res = a.assign(Bag(priors=Bag(tensor=pz)), Bag(bboxes=Bag(tensor=torch.ones(2, gz.shape[1])), labels=torch.zeros(2, dtype=torch.int64)))
        assert res.num_gts == 2 and res.gt_inds.shape == res.labels.shape == res.max_overlaps.shape == (0,) and res.gt_inds.dtype == torch.int64
        assert a.iou_calculator(gz, torch.ones(3, pz.shape[1])).shape == (0, 3)


def test_refusals():
    from mtp_amd import BboxOverlaps2D, MaxIoUAssigner, RBbox2HBboxOverlaps2D, RBboxOverlaps2D, batched_nms, bbox_overlaps, nms, nms_rotated, ops
    b, s = torch.ones(3, 4), torch.ones(3)
    with pytest.raises(NotImplementedError):
        nms(b, s, 0.5, offset=1)
    with pytest.raises(NotImplementedError):
        bbox_overlaps(b, b, mode="giou")
    with pytest.raises(NotImplementedError):
        bbox_overlaps(torch.ones(2, 3, 4), torch.ones(2, 3, 4))
    for cls in (BboxOverlaps2D, RBboxOverlaps2D, RBbox2HBboxOverlaps2D):
        with pytest.raises(NotImplementedError):
            cls(dtype="fp16")
    a = MaxIoUAssigner(0.5, 0.5, ignore_iof_thr=0.5)
    with pytest.raises(NotImplementedError):
        a.assign(Bag(priors=b), Bag(bboxes=b, labels=torch.zeros(3, dtype=torch.int64)), Bag(bboxes=b))
    n = ops.NMS_MAX_BOXES + 1
    assert ops.NMS_MAX_BOXES == 32768
    with pytest.raises(ValueError):
        nms(torch.ones(n, 4), torch.ones(n), 0.5)
    with pytest.raises(ValueError):
        nms_rotated(torch.ones(n, 5), torch.ones(n), 0.1)
    with pytest.raises(ValueError):
        batched_nms(torch.ones(n, 4), torch.ones(n), torch.zeros(n, dtype=torch.int64), dict(type="nms", iou_threshold=0.5))
    with pytest.raises(NotImplementedError):
        batched_nms(b, s, torch.zeros(3, dtype=torch.int64), dict(type="soft_nms", iou_threshold=0.5))
    with pytest.raises(RuntimeError):          # no CPU fallback: boxes on the host reach the kernels' wrapper and are refused there
        bbox_overlaps(b, b)
