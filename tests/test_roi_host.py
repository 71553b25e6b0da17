"""CPU: the inputs of the oriented-RoI-head tests meet their conditions (tests/roi_cases.py, from the float64 reference alone), the restatement
tests/roi_ref.py agrees with a brute-force RoIAlignRotated and with finite differences, the coder inverts itself, and the Python surface carries the
reference's names, state-dict keys and refusals.  Fixture f23 (the reference's own RoI head run in float64, tests/golden/make_oriented_roi.py)
regenerates bit for bit where the reference is at hand, holds the inputs and the sampler's choice of roi_cases, and roi_ref agrees with it on every
recorded value: targets, losses, accuracy, gradients, detections.  No GPU."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import roi_cases as RC
import roi_ref as R
from mtp_amd import MODELS, TASK_UTILS, _lib


# ------------------------------------------------------------------------------------------------------------------- the cases
def test_align_case_meets_its_conditions():
    maps, rois = RC.align_case()
    assert RC.align_condition((maps, rois)) and sorted(maps) == [RC.C, RC.C_WIDE]
    lv = R.map_levels(rois, 4, RC.FINEST)
    raw = np.floor(np.log2(np.sqrt(rois[:, 3].astype(np.float64) * rois[:, 4]) / RC.FINEST + 1e-6))
    assert set(lv.tolist()) == {0, 1, 2, 3} and raw.max() > 3 and raw.min() < 0      # every level and both clamped ends
    out = R.roi_align(maps[RC.C], rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST)
    assert not out[7].any() and out[6].any() and (out[6] == 0).any()      # wholly outside: zeros; partly outside: some bins
    assert rois[8, 3] / RC.STRIDES[0] < 1 and rois[8, 4] / RC.STRIDES[0] < 1      # smaller than a pixel
    assert abs(rois[9, 5]) < 0.01 and abs(abs(rois[10, 5]) - np.pi / 2) < 0.01 and abs(abs(rois[11, 5]) - np.pi / 2) < 0.01 and rois[10, 5] > 0 > rois[11, 5]


@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_head_case_meets_its_conditions(name):
    c = RC.case(name)
    assert RC.condition(name, c)
    sm, _ = RC.sampling(c)
    counts = RC.SHAPES[name][2]
    assert [len(g) for g in c["gts"]] == list(counts) and all(len(p) == RC.NUM_PROP for p in c["props"])
    for q, k in zip(sm, counts):
        assert len(q["pos"]) == (int(RC.NUM * RC.POS_FRACTION) if k else 0) and (q["gt_inds"][:k] == np.arange(1, k + 1)).all()
    if name == "sq128":
        assert any(len(q["pos"]) + len(q["neg"]) < RC.NUM for q in sm)      # padded slots
    else:
        assert len(sm[1]["pos"]) == 0 and len(sm[1]["neg"]) == RC.NUM      # the image without gts
    ref = RC.reference(name)
    assert ref["x"].shape == (RC.BATCH * RC.NUM, RC.C, RC.P, RC.P) and not ref["x"][~ref["lists"]["valid"]].any()
    assert 0 < float(ref["loss"]["acc"]) < 100 and float(ref["loss"]["loss_cls"]) > 0 and float(ref["loss"]["loss_bbox"]) > 0


# ------------------------------------------------------------------------------------------------------------------- fixture f23
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_f23_regenerates(tmp_path):
    gen = os.path.join(GOLDEN, "make_oriented_roi.py")
    ref_dir = [l.split('"')[1] for l in open(os.path.join(GOLDEN, "make_oriented_rpn.py")) if l.startswith("REF_DIR")][0]
    if not os.path.isdir(ref_dir):
        pytest.skip("the reference is not on this machine")
    out = str(tmp_path / "f23.npz")
    subprocess.run([sys.executable, gen, out], check=True, capture_output=True)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "f23_oriented_roi.npz"), "rb").read()


@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_roi_ref_and_cases_vs_f23(golden, name):
    """the reference's control flow and the restatement agree: the inputs, the sampler's choice (gts prepended), rois, RoI features, labels and
    targets, losses and acc with avg_factor = the number of sampled RoIs, every gradient, and the kept detections of three configurations"""
    f, c, ref, p = golden("f23_oriented_roi.npz"), RC.case(name), RC.reference(name), name + "."
    h = hashlib.sha256()
    for a in c["feats"] + c["gts"] + c["labels"] + c["props"] + [c["W"][k] for k in sorted(c["W"])]:
        h.update(np.ascontiguousarray(a).tobytes())
    assert bytes(f[p + "inputs_sha256"]) == h.digest() and int(f[p + "seed"]) == RC.SEEDS[name]
    for b, q in enumerate(RC.sampling(c)[0]):
        i = "%simage%d." % (p, b)
        assert f[i + "pos_inds"].tolist() == q["pos"].tolist() and f[i + "neg_inds"].tolist() == q["neg"].tolist() and f[i + "pos_gt"].tolist() == q["pos_gt"].tolist()
    L, v = ref["lists"], ref["lists"]["valid"]
    err = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max()) if np.size(a) else 0.0      # noqa: E731
    assert f[p + "rois"].shape == (int(v.sum()), 6) and err(f[p + "rois"], L["rois"][v]) == 0 and err(f[p + "bbox_feats"], ref["x"][v]) < 1e-12
    assert np.array_equal(f[p + "labels"], ref["loss"]["labels"][v]) and err(f[p + "bbox_targets"], ref["loss"]["targets"][v]) < 1e-12
    assert f[p + "label_weights"].all() and np.array_equal(f[p + "bbox_weights"].any(1), f[p + "labels"] < RC.K)
    assert err(f[p + "cls_score"], ref["cls"][v]) < 1e-12 and err(f[p + "bbox_pred"], ref["reg"][v]) < 1e-12
    for k in ("loss_cls", "loss_bbox", "acc"):
        assert abs(float(f[p + k]) - float(ref["loss"][k])) < 1e-12, k
    for k, g in ref["G"].items():
        assert err(f[p + "grad." + k], g) < 1e-13, k
    for l, g in enumerate(ref["dfeats"]):
        assert err(f["%slevel%d.dfeat" % (p, l)], g) < 1e-14
    assert err(f[p + "d_bbox_feats"], ref["dx"][v]) < 1e-8      # (recorded in float32)
    assert err(f[p + "test.cls_score"], ref["tcls"]) < 1e-12 and err(f[p + "test.bbox_pred"], ref["treg"]) < 1e-12
    for tag in ("det", "det_thr", "det_cut"):
        for b in range(RC.BATCH):
            keep, boxes, scores, labels = ref["dets"][tag][b][:4]
            q = "%s%s.image%d." % (p, tag, b)
            assert f[q + "keep"].tolist() == keep.tolist() and f[q + "labels"].tolist() == labels.tolist()
            assert err(f[q + "bboxes"], boxes) < 1e-11 and err(f[q + "scores"], scores) < 1e-13


# ------------------------------------------------------------------------------------------------------------------- the restatement
def test_roi_ref_forward_against_brute_force():
    maps, rois = RC.align_case()
    lv = R.map_levels(rois, 4, RC.FINEST)
    out = R.roi_align(maps[RC.C_WIDE], rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST)
    for r in (0, 1, 3, 6, 7, 8, 10, 11, 15):
        m = maps[RC.C_WIDE][lv[r]][int(rois[r, 0])].astype(np.float64)
        assert np.abs(out[r] - R.roi_align_one(m, rois[r].astype(np.float64), RC.STRIDES[lv[r]], RC.P, RC.S, RC.CLOCKWISE)).max() < 1e-12, r
    anti = R.roi_align(maps[RC.C], rois[:4], RC.STRIDES, RC.P, RC.S, False, RC.FINEST)      # clockwise negates theta
    flip = rois[:4].copy()
    flip[:, 5] *= -1
    assert np.array_equal(anti, R.roi_align(maps[RC.C], flip, RC.STRIDES, RC.P, RC.S, True, RC.FINEST))


def test_roi_ref_backward_against_finite_differences():
    maps, rois = RC.align_case()
    maps = [m.astype(np.float64) for m in maps[RC.C]]
    rng = np.random.default_rng(3)
    dout = rng.normal(0, 1, (len(rois), RC.C, RC.P, RC.P))
    args = (rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST)
    grads = R.roi_align_bwd(dout, [m.shape for m in maps], *args)
    f = lambda ms: float((R.roi_align(ms, *args) * dout).sum())      # noqa: E731
    for l, g in enumerate(grads):
        touched = np.argwhere(g != 0)
        assert len(touched)
        for idx in list(touched[rng.integers(0, len(touched), 3)]) + [np.argwhere(g == 0)[0]]:
            up, dn = [m.copy() for m in maps], [m.copy() for m in maps]
            up[l][tuple(idx)] += 0.5
            dn[l][tuple(idx)] -= 0.5
            assert abs((f(up) - f(dn)) - g[tuple(idx)]) < 1e-9 * max(1.0, abs(g[tuple(idx)]))      # the operator is linear in the map


def test_coder_inverts_itself_and_clamps():
    rng = np.random.default_rng(9)
    n = 400
    p = np.concatenate([rng.uniform(20, 100, (n, 2)), rng.uniform(8, 60, (n, 2)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1)
    g = np.concatenate([p[:, :2] + rng.uniform(-6, 6, (n, 2)), rng.uniform(8, 60, (n, 2)), rng.uniform(-np.pi / 2 + 0.01, np.pi / 2 - 0.01, (n, 1))], 1)
    g[:, 2:4] = np.sort(g[:, 2:4], 1)[:, ::-1]      # 'le90': w >= h
    fine = (g[:, 2] - g[:, 3] > 1e-3 * g[:, 2]) & (R.angle_margins(p, g)[0] > 1e-3)      # away from the swap boundary
    assert fine.sum() > 300
    back = R.decode(p[fine], R.encode(p[fine], g[fine], RC.MEANS, RC.STDS), RC.MEANS, RC.STDS)
    assert np.abs(back - g[fine]).max() < 1e-9
    # both clamps, and a prior against itself: zero deltas, the box again
    d = np.zeros((3, 5))
    d[0, 2], d[1, 3] = 99.0, -99.0
    out = R.decode(p[:3], d, RC.MEANS, RC.STDS)
    assert abs(max(out[0, 2:4]) / p[0, 2] - 1000 / 16) < 1e-9 and abs(min(out[1, 2:4]) / p[1, 3] - 16 / 1000) < 1e-12
    q = g[fine][:5]
    assert np.abs(R.encode(q, q, RC.MEANS, RC.STDS)).max() == 0 and np.abs(R.decode(q, np.zeros((5, 5)), RC.MEANS, RC.STDS) - q).max() < 1e-12


# ------------------------------------------------------------------------------------------------------------------- the Python surface
ROI_HEAD = dict(
    type="MTP_RD_StandardRoIHead",
    bbox_roi_extractor=dict(type="RotatedSingleRoIExtractor", roi_layer=dict(type="RoIAlignRotated", out_size=7, sample_num=2, clockwise=True), out_channels=256,
                            featmap_strides=[4, 8, 16, 32]),
    bbox_head=dict(type="MTP_RD_Shared2FCBBoxHead", predict_box_type="rbox", in_channels=256, fc_out_channels=64, roi_feat_size=7,
                   reg_predictor_cfg=dict(type="mmdet.Linear"), cls_predictor_cfg=dict(type="mmdet.Linear"),
                   bbox_coder=dict(type="mmrotate.DeltaXYWHTRBBoxCoder", angle_version="le90", norm_factor=None, edge_swap=True, proj_xy=True,
                                   target_means=(.0, .0, .0, .0, .0), target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)),
                   reg_class_agnostic=True, loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                   loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=1.0, loss_weight=1.0)),
    train_cfg=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False,
                                 iou_calculator=dict(type="mmrotate.RBboxOverlaps2D"), ignore_iof_thr=-1),
                   sampler=dict(type="RandomSampler", num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1, debug=False),
    test_cfg=dict(nms_pre=2000, min_bbox_size=0, score_thr=0.05, nms=dict(type="nms_rotated", iou_threshold=0.1), max_per_img=2000))


def _with(path, **kw):
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in ROI_HEAD.items()}
    if path:
        cfg[path] = dict(cfg[path], **kw)
    else:
        cfg.update(kw)
    return cfg


def test_registry_names_and_state_dict_keys():
    for reg, names in ((MODELS, ("StandardRoIHead", "MTP_RD_StandardRoIHead", "Shared2FCBBoxHead", "MTP_RD_Shared2FCBBoxHead", "RotatedSingleRoIExtractor",
                                 "mmrotate.RotatedSingleRoIExtractor", "RoIAlignRotated")),
                       (TASK_UTILS, ("DeltaXYWHTRBBoxCoder", "mmrotate.DeltaXYWHTRBBoxCoder"))):
        for n in names:
            assert reg.get(n) is not None, n
    head = MODELS.build(ROI_HEAD)      # the reference's dict as it stands: no num_classes
    shared = ["bbox_head.shared_fcs.%d.%s" % (i, k) for i in (0, 1) for k in ("bias", "weight")]
    assert sorted(head.state_dict()) == shared and head.bbox_head.num_classes is None
    assert head.bbox_head.cls_last_dim == head.bbox_head.reg_last_dim == 64 and tuple(head.bbox_head.shared_fcs[0].weight.shape) == (64, 256 * 49)
    assert head.add_gt_as_proposals and head.bbox_sampler.add_gt_as_proposals is False and head.bbox_sampler.num == 512
    assert head.bbox_roi_extractor.num_inputs == 4 and head.bbox_roi_extractor.finest_scale == 56 and head.bbox_head.bbox_coder.encode_size == 5
    tuned = MODELS.build(_with("bbox_head", num_classes=15))
    assert sorted(tuned.state_dict()) == sorted(shared + ["bbox_head.fc_%s.%s" % (a, b) for a in ("cls", "reg") for b in ("bias", "weight")])
    assert tuple(tuned.bbox_head.fc_cls.weight.shape) == (16, 64) and tuple(tuned.bbox_head.fc_reg.weight.shape) == (5, 64)
    for m in ("gen_sampling_results", "train_bbox_forward", "test_bbox_generate_roi", "test_bbox_roi_feats", "_bbox_forward", "bbox_loss", "predict_bbox",
              "loss", "predict", "loss_and_grads"):
        assert callable(getattr(head, m)), m


def test_refusals():
    bad = [_with("bbox_head", num_shared_convs=1), _with("bbox_head", with_avg_pool=True), _with("bbox_head", reg_class_agnostic=False),
           _with("bbox_head", reg_decoded_bbox=True), _with("bbox_head", loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=True)),
           _with("bbox_head", loss_bbox=dict(type="mmdet.L1Loss")), _with(None, mask_head=dict(type="FCNMaskHead")), _with(None, shared_head=dict(type="ResLayer")),
           _with("bbox_roi_extractor", roi_layer=dict(type="RoIAlign", output_size=7)),
           _with("bbox_roi_extractor", roi_layer=dict(type="RoIAlignRotated", out_size=7, sample_num=0)),
           _with("bbox_roi_extractor", roi_layer=dict(type="RoIAlignRotated", out_size=7, sample_num=2, aligned=False))]
    for coder in (dict(angle_version="oc"), dict(norm_factor=2), dict(edge_swap=False), dict(proj_xy=False)):
        bad.append(_with("bbox_head", bbox_coder=dict(ROI_HEAD["bbox_head"]["bbox_coder"], **coder)))
    for cfg in bad:
        with pytest.raises(NotImplementedError):
            MODELS.build(cfg)
    with pytest.raises(NotImplementedError):      # the sampler class itself is as it was
        TASK_UTILS.build(dict(type="RandomSampler", num=8, pos_fraction=0.5, add_gt_as_proposals=True))
    head = MODELS.build(ROI_HEAD)
    with pytest.raises(ValueError):      # a head without num_classes takes its predictors per call
        head.bbox_head.predictors()
    none = head.predict([torch.zeros(1, 256, s, s) for s in (32, 16, 8, 4)], [dict(bboxes=torch.zeros(0, 5))], num_classes=3,
                        fc_cls=torch.nn.Linear(64, 4), fc_reg=torch.nn.Linear(64, 5))      # R = 0: empty results, the library untouched
    assert len(none) == 1 and len(none[0].scores) == 0 and tuple(none[0].bboxes.shape) == (0, 5)


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_entries():
    names = ["mtp_roi_align_rotated_fwd", "mtp_roi_align_rotated_entries", "mtp_roi_align_rotated_bwd_entries", "mtp_roi_align_rotated_bwd_gather",
             "mtp_rbox_delta_encode", "mtp_rbox_delta_decode", "mtp_roi_loss_workspace_bytes", "mtp_roi_loss", "mtp_roi_predict"]
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and getattr(lib, n) is not None
    assert C.sizeof(_lib.RoiLevel) == 8 * 9 and _lib.RoiLevel.stride.offset == 40 and _lib.ROI_MAX_LEVELS == 8
    assert lib.mtp_roi_align_rotated_entries(3, 7, 2) == 3 * 49 * 4 * 4 and lib.mtp_roi_align_rotated_entries(0, 7, 2) == -1
    assert lib.mtp_roi_loss_workspace_bytes(2, 512) == 2 * 2 * 3 * 4 and lib.mtp_roi_loss_workspace_bytes(2, 0) == -1
    P = 1 << 20      # a non-NULL pointer that is never dereferenced: every call below is refused before it launches
    lv = (_lib.RoiLevel * 1)()
    lv[0].map, lv[0].H, lv[0].W, lv[0].spatial_scale = P, 8, 8, 0.25
    f5 = (C.c_float * 5)(*([1.0] * 5))
    z5 = (C.c_float * 5)(1.0, 1.0, 0.0, 1.0, 1.0)
    assert lib.mtp_roi_align_rotated_fwd(lv, 1, 2, 8, P, None, None, 4, 0, 7, 0, 1, 56.0, P, None, None) == -1      # sample_num 0
    assert lib.mtp_roi_align_rotated_fwd(lv, 1, 2, 8, P, None, None, 4, 0, 40, 2, 1, 56.0, P, None, None) == -1     # more sample points than LDS holds
    assert lib.mtp_roi_align_rotated_fwd(lv, 1, 2, 8, P, None, P, 5, 2, 7, 2, 1, 56.0, P, None, None) == -1         # R no multiple of the group size
    assert lib.mtp_roi_align_rotated_fwd(lv, 9, 2, 8, P, None, None, 4, 0, 7, 2, 1, 56.0, P, None, None) == -1      # too many levels
    assert lib.mtp_roi_align_rotated_bwd_gather(lv, 1, 2, 8, P, P, P, P, 4, 7, 2, 0, None) == -1                    # no gradient map
    assert lib.mtp_rbox_delta_encode(P, P, f5, z5, 4, P, None) == -1 and lib.mtp_rbox_delta_decode(P, P, f5, z5, 4, P, None) == -1      # a zero std
    assert lib.mtp_roi_loss(P, 6, P, 5, 6, P, P, P, 3, P, P, P, 2, 32, f5, f5, 1.0, 1.0, 1.0, P, None, None, P, 1 << 16, None) == -1    # ld_cls <= classes
    assert lib.mtp_roi_loss(P, 8, P, 5, 5, P, P, P, 3, P, P, P, 2, 32, f5, f5, 1.0, 1.0, 1.0, P, P, None, P, 1 << 16, None) == -1      # dcls without dreg
    assert lib.mtp_roi_loss(P, 8, P, 5, 5, P, P, P, 3, P, P, P, 2, 32, f5, f5, 1.0, 1.0, 1.0, P, None, None, P, 8, None) == -1         # workspace too small
    assert lib.mtp_roi_predict(P, 8, P, 4, 5, P, 4, f5, f5, 0.05, P, P, P, None) == -1                                                   # ld_reg < 5
