"""CPU: the box half of Mask R-CNN without a device: the restatement tests/hbox_ref.py against fixture f26 (the reference's own heads) and against a
naive one-element-at-a-time coder, the conditions of tests/hbox_cases.py, registry names, state-dict keys, the refusals by name, empty inputs."""
import math

import numpy as np
import pytest
import torch

import hbox_cases as HC
import hbox_ref as R
from mtp_amd import MODELS, TASK_UTILS, ops
from mtp_amd.dense_heads import RPNHead
from mtp_amd.roi_heads import HBoxRoIHead, HBoxShared2FCBBoxHead, MaskRoIHead, Shared2FCBBoxHead
from mtp_amd.task_modules import DeltaXYWHBBoxCoder

F64, F32 = np.float64, np.float32


# ------------------------------------------------------------------------------------------------------------------- the coder, naively
def encode_one(p, g, means, stds):
    px, py, pw, ph = (p[0] + p[2]) / 2, (p[1] + p[3]) / 2, p[2] - p[0], p[3] - p[1]
    gx, gy, gw, gh = (g[0] + g[2]) / 2, (g[1] + g[3]) / 2, g[2] - g[0], g[3] - g[1]
    d = [(gx - px) / pw, (gy - py) / ph, math.log(gw / pw), math.log(gh / ph)]
    return [(d[i] - means[i]) / stds[i] for i in range(4)]


def decode_one(p, raw, means, stds, max_shape=None, clip=16 / 1000):
    d = [raw[i] * stds[i] + means[i] for i in range(4)]
    mr = abs(math.log(clip))
    dw, dh = min(max(d[2], -mr), mr), min(max(d[3], -mr), mr)
    px, py, pw, ph = (p[0] + p[2]) / 2, (p[1] + p[3]) / 2, p[2] - p[0], p[3] - p[1]
    gx, gy, gw, gh = px + pw * d[0], py + ph * d[1], pw * math.exp(dw), ph * math.exp(dh)
    box = [gx - gw / 2, gy - gh / 2, gx + gw / 2, gy + gh / 2]
    if max_shape is not None:
        h, w = max_shape
        box = [min(max(box[0], 0), w), min(max(box[1], 0), h), min(max(box[2], 0), w), min(max(box[3], 0), h)]
    return box


def test_restated_coder_against_the_naive_one():
    rng = np.random.default_rng(3)
    n = 300
    c, wh = rng.uniform(5, 60, (n, 2)), rng.uniform(2, 50, (n, 2))
    p = np.concatenate([c - wh / 2, c + wh / 2], 1)
    c2, wh2 = c + rng.uniform(-8, 8, (n, 2)), wh * rng.uniform(0.3, 3, (n, 2))
    g = np.concatenate([c2 - wh2 / 2, c2 + wh2 / 2], 1)
    d = rng.normal(0, 1, (n, 4)) * [3, 3, 12, 12]
    for means, stds in (((0, 0, 0, 0), (1, 1, 1, 1)), (HC.ROI_MEANS, HC.ROI_STDS), ((0.1, -0.2, 0.3, 0.05), (0.5, 0.5, 0.25, 0.3))):
        want = np.array([encode_one(p[i], g[i], means, stds) for i in range(n)])
        assert np.abs(R.encode(p, g, means, stds) - want).max() < 1e-12
        for ms in (None, (40, 56)):
            want = np.array([decode_one(p[i], d[i], means, stds, ms) for i in range(n)])
            got = R.decode(p, d, means, stds, ms)
            assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
        table = np.array([[64, 64], [40, 56], [48, 32]], F64)[rng.integers(0, 3, n)]      # a per-row table
        want = np.array([decode_one(p[i], d[i], means, stds, table[i]) for i in range(n)])
        assert np.abs(R.decode(p, d, means, stds, table) - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert (np.abs(d[:, 2:] * 0.2) > abs(math.log(0.016))).any()      # the clamp acted
    back = R.decode(p, R.encode(p, g, HC.ROI_MEANS, HC.ROI_STDS), HC.ROI_MEANS, HC.ROI_STDS)      # within the clamp the coder inverts itself
    inside = (np.abs(np.log(wh2 / wh)) < 4).all(1)
    assert inside.sum() > 200 and np.abs(back[inside] - g[inside]).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_case_conditions(name):
    """the pinned seed meets every condition, and the float32 run takes every decision as the float64 run does"""
    assert HC.condition(name, HC.case(name))
    r, y = HC.reference(name), HC.yardstick(name)
    for a, b in zip(r["rpn"]["props"], y["rpn"]["props"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3][2], b[3][2]) and np.array_equal(a[3][3], b[3][3])      # kept, level ids, valid
    for k in ("n_pos", "n_neg", "sample_gt", "valid"):
        assert np.array_equal(r["roi"]["lists"][k], y["roi"]["lists"][k])
    for t in ("reference", "encoded"):
        assert np.array_equal(r["roi"]["loss"][t]["labels"], y["roi"]["loss"][t]["labels"]) and abs(float(r["roi"]["loss"][t]["acc"]) - float(y["roi"]["loss"][t]["acc"])) < 1e-4      # the same hits
        assert np.array_equal(np.sign(r["roi"]["loss"][t]["dreg"]), np.sign(y["roi"]["loss"][t]["dreg"]))
    for tag in ("plain", "rescale", "top"):
        for a, b in zip(r["dets"][tag], y["dets"][tag]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4] > HC.RCNN["score_thr"], b[4] > HC.RCNN["score_thr"])
    assert np.array_equal(r["mask"]["train"]["targets"], y["mask"]["train"]["targets"])
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(r["mask"]["pasted"], y["mask"]["pasted"]))
    gts = sum(HC.SHAPES[name])
    assert (r["roi"]["lists"]["n_pos"] > 0).any() == (gts > 0)
    if name == "full":
        L = r["roi"]["loss"]
        assert L["reference"]["loss_bbox"] > 0 and L["encoded"]["loss_bbox"] > 0 and L["reference"]["loss_bbox"] != L["encoded"]["loss_bbox"]
        assert L["reference"]["loss_cls"] == L["encoded"]["loss_cls"]      # the targets differ, the labels do not


def test_planted_maps():
    assert HC.planted_condition(HC.planted())


def test_nms_pre_bites_on_the_fine_levels_only():
    counts = [min(HC.PROPOSAL["nms_pre"], h * w * HC.A) for h, w in HC.SIZES]
    assert counts == [12, 12, 12, 12, 3] and [h * w * HC.A for h, w in HC.SIZES] == [768, 192, 48, 12, 3]


def test_restated_losses_in_closed_form():
    """hbox_ref.roi_loss on two rows worked out by hand: the reference's target (1.0) and mmdet's (the encoded deltas)"""
    K = 2
    cls = np.array([[0.0, math.log(3.0), 0.0], [0.0, 0.0, math.log(2.0)]])      # softmax (1/5, 3/5, 1/5) and (1/4, 1/4, 1/2)
    reg = np.array([[9, 9, 9, 9, 1.5, 0.5, 1.0, 3.0], [7, 7, 7, 7, 7, 7, 7, 7]], F64)
    rois, gts = np.array([[0, 0, 10, 10], [5, 5, 9, 9]], F64), np.array([[1, 0, 11, 10]], F64)
    args = (cls, reg, K, rois, gts, np.array([1]), np.array([[0, -1]]), [1], [1], (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2))
    a = R.roi_loss(*args, reg_target="reference")
    assert abs(a["loss_cls"] - (math.log(5 / 3) + math.log(2)) / 2) < 1e-12 and a["acc"] == 100.0
    assert abs(a["loss_bbox"] - (0.5 + 0.5 + 0.0 + 2.0) / 2) < 1e-12
    assert a["dreg"][0].tolist() == [0, 0, 0, 0, 0.5, -0.5, 0.0, 0.5] and not a["dreg"][1].any()      # L1: sign / R_total, 0 at equality; dense zeros
    b = R.roi_loss(*args, reg_target="encoded")      # encode: dx = 1 / 10 / 0.1 = 1, the rest 0
    assert abs(b["loss_bbox"] - (0.5 + 0.5 + 1.0 + 3.0) / 2) < 1e-12 and b["targets"][0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert a["labels"].tolist() == [1, 2] and np.abs(a["dcls"][0] - (np.array([1 / 5, 3 / 5, 1 / 5]) - [0, 1, 0]) / 2).max() < 1e-12
    z = R.roi_loss(cls, reg, K, rois, gts, np.array([1]), np.array([[0, -1]]), [0], [0], (0, 0, 0, 0), (1, 1, 1, 1))      # R_total = 0
    assert z["loss_cls"] == 0 and z["loss_bbox"] == 0 and z["acc"] == 0 and not z["dcls"].any() and not z["dreg"].any()


# ------------------------------------------------------------------------------------------------------------------- fixture f26
def close(a, b, tol=1e-9):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape and (a.size == 0 or np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_restatement_against_the_reference(golden, name):
    """fixture f26, the reference's own rpn_head.py / base_bbox_head.py / bbox_head.py / roi_head.py in float64, against hbox_ref chained by
    hbox_cases.run: sampled indices, kept proposals and detections exactly, every float to 1e-9"""
    import hashlib
    f, r, c = golden("f26_hbox_half.npz"), HC.reference(name), HC.case(name)
    p = name + "."
    h = hashlib.sha256()
    for a in c["feats"] + c["gts"] + c["labels"] + [c[g][k] for g in ("rpn", "roi") for k in sorted(c[g])]:
        h.update(np.ascontiguousarray(a).tobytes())
    assert f[p + "inputs_sha256"].tobytes() == h.digest() and int(f[p + "seed"]) == HC.SEEDS[name]      # the fixture is of these inputs
    close(f[p + "rpn.loss_cls"], r["rpn"]["loss_cls"]), close(f[p + "rpn.loss_bbox"], r["rpn"]["loss_bbox"])
    for b in range(HC.BATCH):
        for stage in ("rpn", "roi"):
            q, s = "%s%s.image%d." % (p, stage, b), r[stage]["samples"][b]
            assert f[q + "pos_inds"].tolist() == s["pos"].tolist() and f[q + "neg_inds"].tolist() == s["neg"].tolist() and f[q + "pos_gt"].tolist() == s["pos_gt"].tolist()
        close(f["%srpn.image%d.bbox_targets" % (p, b)], r["rpn"]["targets"][b])      # the reference's get_targets, on the positives
        q = "%srpn.prop.image%d." % (p, b)
        keep, bx, sc, _ = r["rpn"]["props"][b]
        assert f[q + "keep"].tolist() == keep.tolist()
        close(f[q + "bboxes"], bx), close(f[q + "scores"], sc)
        every = R.rpn_proposals([m[b] for m in r["rpn"]["cls"]], [m[b] for m in r["rpn"]["reg"]], HC.priors(), HC.SIZES, HC.A, HC.RPN_MEANS, HC.RPN_STDS, HC.IMG,
                                HC.PROPOSAL["nms_pre"], HC.PROPOSAL["max_per_img"], HC.PROPOSAL["nms"]["iou_threshold"], -1)
        assert f["%srpn.prop_all.image%d.keep" % (p, b)].tolist() == every[0].tolist()      # min_bbox_size -1: nothing dropped for its size
        for tag, mine in (("det", "plain"), ("det_rescale", "rescale")):
            q, d = "%s%s.image%d." % (p, tag, b), r["dets"][mine][b]
            assert f[q + "keep"].tolist() == d[0].tolist() and f[q + "labels"].tolist() == d[3].tolist()
            close(f[q + "bboxes"], d[1]), close(f[q + "scores"], d[2])
    for k in r["rpn"]["G"]:
        close(f[p + "rpn.grad." + k], r["rpn"]["G"][k])
    for l in range(len(HC.SIZES)):
        close(f["%srpn.level%d.dfeat" % (p, l)], r["rpn"]["dfeats"][l].reshape(-1)[::3])
    for k in ("loss_cls", "loss_bbox", "acc"):      # the box loss as the reference computes it: towards the target 1
        close(f[p + "roi." + k], r["roi"]["loss"]["reference"][k])
    valid, enc = r["roi"]["lists"]["valid"], r["roi"]["loss"]["encoded"]      # the reference's get_targets: labels, and the deltas 'encoded' regresses to
    assert f[p + "roi.labels"].tolist() == enc["labels"][valid].tolist() and (f[p + "roi.bbox_weights"].any(1) == (f[p + "roi.labels"] < HC.K)).all()
    close(f[p + "roi.bbox_targets"], enc["targets"][valid])
    for k, g in r["roi"]["G"].items():
        close(f[p + "roi.grad." + k], g.reshape(-1)[::3] if g.size > 4096 else g)
    for l in range(len(HC.ROI_STRIDES)):
        close(f["%sroi.level%d.dfeat" % (p, l)], r["roi"]["dfeats"][l].reshape(-1)[::3])
    if name == "full":      # the reference's target is 1, not the encoded deltas: the two restated losses differ and the fixture has the former
        assert abs(float(f[p + "roi.loss_bbox"]) - float(r["roi"]["loss"]["encoded"]["loss_bbox"])) > 1e-3


# ------------------------------------------------------------------------------------------------------------------- registries, keys, refusals
def rpn_cfg(**kw):
    return dict(dict(type="MTP_IS_RPNHead", in_channels=8, feat_channels=8,
                     anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                     bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
                     loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0)), **kw)


def head_cfg(**kw):
    return dict(dict(type="MTP_IS_Shared2FCBBoxHead", in_channels=8, fc_out_channels=16, roi_feat_size=7,
                     bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2]), reg_class_agnostic=False,
                     loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0)), **kw)


def roi_cfg(**kw):
    return dict(dict(type="MTP_IS_BBoxRoIHead",
                     bbox_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0), out_channels=8,
                                             featmap_strides=[4, 8, 16, 32]),
                     bbox_head=head_cfg()), **kw)


def test_registry_names_and_state_dict_keys():
    assert MODELS.get("MTP_IS_RPNHead") is RPNHead and MODELS.get("RPNHead") is RPNHead
    assert MODELS.get("MTP_IS_Shared2FCBBoxHead") is HBoxShared2FCBBoxHead and MODELS.get("MTP_IS_BBoxRoIHead") is HBoxRoIHead
    assert MODELS.get("Shared2FCBBoxHead") is Shared2FCBBoxHead and MODELS.get("MTP_RD_Shared2FCBBoxHead") is Shared2FCBBoxHead      # the oriented class
    assert MODELS.get("MTP_IS_StandardRoIHead") is MaskRoIHead      # the mask half keeps its name
    assert TASK_UTILS.get("DeltaXYWHBBoxCoder") is DeltaXYWHBBoxCoder and TASK_UTILS.get("mmdet.DeltaXYWHBBoxCoder") is DeltaXYWHBBoxCoder
    rpn = MODELS.build(rpn_cfg())
    assert sorted(rpn.state_dict()) == ["rpn_cls.bias", "rpn_cls.weight", "rpn_conv.bias", "rpn_conv.weight", "rpn_reg.bias", "rpn_reg.weight"]
    assert tuple(rpn.rpn_reg.weight.shape) == (12, 8, 1, 1) and tuple(rpn.rpn_cls.weight.shape) == (3, 8, 1, 1) and rpn.bbox_coder.encode_size == 4
    own, bare = MODELS.build(head_cfg(num_classes=3)), MODELS.build(head_cfg())
    shared = ["shared_fcs.%d.%s" % (i, k) for i in (0, 1) for k in ("bias", "weight")]
    assert sorted(bare.state_dict()) == shared and sorted(own.state_dict()) == sorted(shared + ["fc_cls.bias", "fc_cls.weight", "fc_reg.bias", "fc_reg.weight"])
    assert tuple(own.fc_cls.weight.shape) == (4, 16) and tuple(own.fc_reg.weight.shape) == (12, 16) and own.reg_target == "reference"
    assert MODELS.build(head_cfg(reg_target="encoded")).reg_target == "encoded"
    assert [own.reg_col(k) for k in (1, 2, 3, 4, 15)] == [4, 4, 4, 8, 16]
    roi = MODELS.build(roi_cfg())
    assert isinstance(roi.bbox_head, HBoxShared2FCBBoxHead) and roi.with_bbox and not roi.with_mask and roi.BOX_DIM == 4
    assert sorted(roi.state_dict()) == ["bbox_head." + k for k in shared]
    coder = DeltaXYWHBBoxCoder(target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2))
    assert coder.encode_size == 4 and coder.means == (0.0, 0.0, 0.0, 0.0) and coder.stds == (0.1, 0.1, 0.2, 0.2)
    assert ops.HROI_TARGET == {"reference": 0, "encoded": 1} and ops.HBOX_DELTAS == 4


def test_refusals_by_name():
    for kw, word in ((dict(clip_border=False), "clip_border"), (dict(add_ctr_clamp=True), "add_ctr_clamp"), (dict(use_box_type=True), "use_box_type")):
        with pytest.raises(NotImplementedError, match=word):
            DeltaXYWHBBoxCoder(**kw)
    with pytest.raises(ValueError):
        DeltaXYWHBBoxCoder(target_stds=(1, 1, 0, 1))
    with pytest.raises(NotImplementedError, match="num_convs"):
        MODELS.build(rpn_cfg(num_convs=2))
    with pytest.raises(NotImplementedError, match="L1Loss"):
        MODELS.build(rpn_cfg(loss_bbox=dict(type="SmoothL1Loss", beta=0.1)))
    with pytest.raises(NotImplementedError, match="four deltas"):
        MODELS.build(rpn_cfg(bbox_coder=dict(type="MidpointOffsetCoder", angle_version="le90", target_means=[0.0] * 6, target_stds=[1.0] * 6)))
    with pytest.raises(NotImplementedError, match="reg_class_agnostic"):
        MODELS.build(head_cfg(reg_class_agnostic=True))
    with pytest.raises(NotImplementedError, match="L1Loss"):
        MODELS.build(head_cfg(loss_bbox=dict(type="SmoothL1Loss", beta=1.0)))
    with pytest.raises(ValueError, match="reg_target"):
        MODELS.build(head_cfg(reg_target="ones"))
    with pytest.raises(NotImplementedError, match="reg_decoded_bbox"):
        MODELS.build(head_cfg(reg_decoded_bbox=True))
    with pytest.raises(NotImplementedError, match="mask half"):
        MODELS.build(roi_cfg(mask_head=dict(type="MTP_IS_FCNMaskHead")))
    with pytest.raises(NotImplementedError):      # the mask half still refuses the box half: the two compose through data
        MODELS.build(dict(type="MTP_IS_StandardRoIHead", bbox_head=head_cfg(), mask_roi_extractor=roi_cfg()["bbox_roi_extractor"], mask_head=dict(type="MTP_IS_FCNMaskHead")))
    with pytest.raises(NotImplementedError):      # the oriented head still refuses the per-class regression
        MODELS.build(dict(type="Shared2FCBBoxHead", in_channels=8, fc_out_channels=16, reg_class_agnostic=False))
    head = MODELS.build(head_cfg())
    with pytest.raises(ValueError, match="num_classes"):
        head.predictors()
    with pytest.raises(ValueError, match="4 \\* num_classes"):
        head.predictors(3, torch.nn.Linear(16, 4), torch.nn.Linear(16, 4))


def test_wrappers_refuse_before_the_library():
    """shape and dtype errors are raised on the host, on CPU tensors: nothing reaches a kernel"""
    z = torch.zeros
    with pytest.raises(ValueError, match="4 means"):
        ops.hbox_delta_encode(z(2, 4), z(2, 4), (0, 0, 0), (1, 1, 1))
    with pytest.raises(TypeError):
        ops.hbox_delta_encode(z(2, 5), z(2, 5), (0,) * 4, (1,) * 4)
    with pytest.raises(ValueError, match="image_ids"):
        ops.hbox_delta_decode(z(2, 4), z(2, 4), (0,) * 4, (1,) * 4, image_ids=z(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="reg_target"):
        ops.hroi_loss(z(4, 3), z(4, 8), 2, z(4, 4), z(1, 4), z(1, dtype=torch.int64), z(2, 2, dtype=torch.int64), z(2, dtype=torch.int64), z(2, dtype=torch.int64),
                      (0,) * 4, (1,) * 4, reg_target="mmdet")
    with pytest.raises(ValueError):
        ops.hroi_predict(z(0, 3), z(0, 8), 2, z(0, 5), (0,) * 4, (1,) * 4, z(1, 2))


def test_empty_inputs_touch_no_library():
    coder = DeltaXYWHBBoxCoder()
    assert tuple(coder.encode(torch.zeros(0, 4), torch.zeros(0, 4)).shape) == (0, 4)
    assert tuple(coder.decode(torch.zeros(0, 4), torch.zeros(0, 4), max_shape=(64, 64)).shape) == (0, 4)
    own, bare = MODELS.build(head_cfg(num_classes=3)), MODELS.build(head_cfg())
    cls, reg = own(torch.zeros(0, 8, 7, 7))
    assert tuple(cls.shape) == (0, 4) and tuple(reg.shape) == (0, 12)
    x_cls, x_reg = bare(torch.zeros(0, 8, 7, 7))
    assert tuple(x_cls.shape) == (0, 16) and x_cls is x_reg
    metas = [dict(img_shape=(64, 64), scale_factor=(1.0, 1.0))] * 2
    res = own.predict_by_feat(torch.zeros(0, 5), None, None, metas, rcnn_test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=100))
    assert len(res) == 2 and all(tuple(r.bboxes.shape) == (0, 4) and r.labels.dtype == torch.int64 for r in res)
    raw = own.predict_by_feat(torch.zeros(0, 5), None, None, metas)
    assert all(tuple(r.bboxes.shape) == (0, 12) and tuple(r.scores.shape) == (0, 4) for r in raw)
    roi = MODELS.build(roi_cfg(test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=100)))
    out = roi.predict([torch.zeros(2, 8, s, s) for s in (16, 8, 4, 2)], [dict(bboxes=torch.zeros(0, 4))] * 2, metas, num_classes=3, fc_cls=torch.nn.Linear(16, 4),
                      fc_reg=torch.nn.Linear(16, 12))
    assert len(out) == 2 and all(len(r.scores) == 0 for r in out)
