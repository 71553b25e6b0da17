"""CPU: the mask branch's host side.  tests/mask_ref.py (float64) and tests/mask_cases.py against fixture f25, the reference's own mask_head.py and
roi_head.py; constructors, state-dict keys and registry names; every refusal; the R = 0 and N = 0 shapes, which never touch the library."""
import hashlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import mask_cases as MC
import mask_ref as MR
from mtp_amd import MODELS, ops
from mtp_amd.ops_roi import RoIAlign, roi_align
from mtp_amd.roi_extractors import SingleRoIExtractor
from mtp_amd.roi_heads import FCNMaskHead, MaskRoIHead, MTP_IS_FCNMaskHead, MTP_IS_StandardRoIHead

CASES = list(MC.SHAPES)


@pytest.fixture(scope="module")
def f25(golden):
    return golden("f25_mask_branch.npz")


def head_cfg(**over):
    cfg = dict(type="MTP_IS_StandardRoIHead",
               mask_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0), out_channels=8,
                                       featmap_strides=[4, 8, 16, 32], finest_scale=16),
               mask_head=dict(type="MTP_IS_FCNMaskHead", num_convs=4, in_channels=8, conv_out_channels=8,
                              loss_mask=dict(type="CrossEntropyLoss", use_mask=True, loss_weight=1.0)),
               train_cfg=dict(mask_size=28, sampler=dict(type="RandomSampler", num=32, pos_fraction=0.25), pos_weight=-1, debug=False),
               test_cfg=dict(mask_thr_binary=0.5))
    cfg.update(over)
    return cfg


# ------------------------------------------------------------------------------------------------------------------- the restatement against f25
@pytest.mark.parametrize("name", CASES)
def test_mask_ref_against_f25(name, f25):
    c = MC.case(name)
    h = hashlib.sha256()
    for a in c["feats"] + [c["bitmaps"], c["rois"], c["sample_gt"], c["labels"], c["n_pos"], c["paste"]["logits"], c["paste"]["boxes"]] \
            + [c["weights"][k] for k in sorted(c["weights"])] + [c["conv_logits"][k] for k in sorted(c["conv_logits"])]:
        h.update(np.ascontiguousarray(a).tobytes())
    assert np.array_equal(np.frombuffer(h.digest(), np.uint8), f25[name + ".digest"]), "the inputs are the ones the fixture was made from"
    assert int(f25[name + ".seed"]) == MC.SHAPES[name]["seed"]
    use, step = MC.in_use(c), int(f25["step"])
    r = MC.run(c)
    thin = (lambda a: a) if name == "base" else (lambda a: a[..., ::step, ::step])
    assert np.array_equal(r["levels"][use], f25[name + ".levels"])
    assert np.array_equal(r["targets"][use], f25[name + ".targets"]) and not r["targets"][~use].any()
    for key, mine in (("mask_feats", thin(r["mask_feats"][use])), ("mask_preds", thin(r["mask_preds"][use])), ("target_avg", r["target_avg"][use]),
                      ("loss_mask", r["loss_mask"])):
        want = f25[name + "." + key]
        assert mine.shape == want.shape and (want.size == 0 or float(np.abs(mine - want).max()) < 1e-12), key
    for k, g in r["grads"].items():
        want = f25["%s.level%s.dfeat" % (name, k[6:])] if k.startswith("feats.") else f25["%s.grad.%s" % (name, k)]
        assert g.shape == want.shape and float(np.abs(g - want).max()) < 1e-12, k
    if use.any():
        assert float(np.abs(f25[name + ".target_avg"] - 0.5).min()) > MC.MARGIN, "no target average near the threshold"
        assert set(np.unique(f25[name + ".levels"]).tolist()) == {0, 1, 2, 3} or name == "one_empty", "every level is hit"
    else:
        assert float(f25[name + ".loss_mask"]) == 0.0 and not any(f25[k].any() for k in f25 if k.startswith(name + ".grad.") or k.endswith(".dfeat") and k.startswith(name))


@pytest.mark.parametrize("name", CASES)
def test_paste_ref_against_f25(name, f25):
    """the reference pastes in float32: its masks are the restatement's bit for bit (no value is near the threshold), its values agree to float32"""
    c = MC.case(name)
    p = c["paste"]
    for rescale, boxes, h, w in MC.paste_frames(c):
        frame = "rescale" if rescale else "scaled"
        v, m = MR.paste(p["logits"], p["labels"], boxes, h, w, MC.THR)
        assert float(np.abs(v - MC.THR).min()) > MC.MARGIN
        assert np.array_equal(m, f25["%s.paste.%s.bool.masks" % (name, frame)].astype(bool))
        _, u8 = MR.paste(p["logits"], p["labels"], boxes, h, w, -1.0)
        assert int(np.abs(u8.astype(np.int64) - f25["%s.paste.%s.u8.masks" % (name, frame)].astype(np.int64)).max()) <= 1
        if name == "base":      # the reference's own float32 values: held like a device result, 4 x the float32 restatement's error, floor 1e-6
            v32, _ = MR.paste(p["logits"], p["labels"], boxes, h, w, MC.THR, ft=np.float32)
            err, e32 = float(np.abs(f25["%s.paste.%s.values" % (name, frame)] - v).max()), float(np.abs(v32 - v).max())
            assert err < max(4 * e32, 1e-6), (err, e32)
    assert (h, w) == (30, 66) and MC.PASTE_HW == (37, 53), "odd sizes, a scale factor other than 1"


def naive_roi_align(m, roi, scale, P, sampling, aligned):
    """mmcv's roi_align_forward for one RoI on one (C, H, W) map, written out as its loop is: one output element, one sample at a time, float64.
    Kept apart from mask_ref on purpose: f25's RoIAlign steps are computed by mask_ref itself, so this is what holds mask_ref to the algorithm."""
    Cc, H, W = m.shape
    off = 0.5 if aligned else 0.0
    x1, y1, x2, y2 = [float(v) * scale - off for v in roi]
    rw, rh = x2 - x1, y2 - y1
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    bh, bw = rh / P, rw / P
    gh = sampling if sampling > 0 else int(np.ceil(rh / P))
    gw = sampling if sampling > 0 else int(np.ceil(rw / P))
    count = max(gh * gw, 1)
    out = np.zeros((Cc, P, P))
    for ph in range(P):
        for pw in range(P):
            for iy in range(gh):
                y = y1 + ph * bh + (iy + 0.5) * bh / gh
                for ix in range(gw):
                    x = x1 + pw * bw + (ix + 0.5) * bw / gw
                    if y < -1.0 or y > H or x < -1.0 or x > W:
                        continue
                    yy, xx = max(y, 0.0), max(x, 0.0)
                    yl, xl = int(yy), int(xx)
                    if yl >= H - 1:
                        yh = yl = H - 1
                        yy = float(yl)
                    else:
                        yh = yl + 1
                    if xl >= W - 1:
                        xh = xl = W - 1
                        xx = float(xl)
                    else:
                        xh = xl + 1
                    ly, lx = yy - yl, xx - xl
                    hy, hx = 1.0 - ly, 1.0 - lx
                    out[:, ph, pw] += hy * hx * m[:, yl, xl] + hy * lx * m[:, yl, xh] + ly * hx * m[:, yh, xl] + ly * lx * m[:, yh, xh]
    return out / count


@pytest.mark.parametrize("aligned,sampling", [(True, 0), (False, 0), (True, 2), (False, 3)])
def test_mask_ref_against_the_naive_loop(aligned, sampling):
    c = MC.case("base")
    rois = np.concatenate([c["rois"][MC.in_use(c)], MC.BIG_ROIS[:2]])
    levels = np.arange(len(rois)) % 4
    levels[-2:] = 0      # the two large boxes on the 16 x 16 map: grids of 11 and 54
    P = 7
    got, _ = MR.roi_align(c["feats"], rois, MC.STRIDES, P, sampling, aligned, MC.FINEST, levels=levels)
    for r, roi in enumerate(rois):
        want = naive_roi_align(c["feats"][levels[r]][int(roi[0])].astype(np.float64), roi[1:], 1.0 / MC.STRIDES[levels[r]], P, sampling, aligned)
        assert float(np.abs(got[r] - want).max()) < 1e-12 * max(1.0, float(np.abs(want).max())), r
    # crop_and_resize: the same loop on a bitmap at scale 1
    bm = c["bitmaps"]
    use = MC.in_use(c)
    boxes, rows = c["boxes"][use][:4], c["sample_gt"].reshape(-1)[use][:4]
    avg, _ = MR.mask_targets(boxes, rows, bm, 12)
    for i, (b, g) in enumerate(zip(boxes, rows)):
        clipped = [np.clip(b[0], 0, MC.IMG), np.clip(b[1], 0, MC.IMG), np.clip(b[2], 0, MC.IMG), np.clip(b[3], 0, MC.IMG)]
        assert float(np.abs(avg[i] - naive_roi_align(bm[g][None].astype(np.float64), clipped, 1.0, 12, 0, True)[0]).max()) < 1e-12, i


@pytest.mark.parametrize("ft", [np.float64, np.float32])
def test_live_samples_by_bisection_equal_a_scan_of_every_sample(ft):
    """mask_ref.live: for grids too long to walk, the samples that can lie inside the map are found by bisection; here every sample is tested"""
    for a, b, scale, size in [(-200.0, 400.0, 0.25, 16), (-1500.0, 1500.0, 0.25, 16), (3.0, 5.0e5, 0.25, 16), (-3.0e5, 40.0, 0.125, 8), (-50.0, 3000.0, 1.0, 300),
                              (100.0, 2.0e6, 1.0, 64), (-2.0e6, 2.0e6, 0.25, 16)]:
        ax = MR.axis(a, b, scale, 14, 0, True, ft)
        assert 8 < ax[2] < 200000
        i = np.arange(ax[2]).astype(ft)
        ok = np.zeros(ax[2], bool)
        for p in range(14):
            v = (ax[0] + ft(p) * ax[1]) + (i + ft(0.5)) * ax[1] / ft(ax[2])
            assert (np.diff(v) >= 0).all(), "nondecreasing in i"
            ok |= (v >= -1) & (v <= size)
        assert list(MR.live(ax, 14, size, ft, whole=8)) == np.nonzero(ok)[0].tolist(), (a, b)
    assert MR.axis(0.0, 6.0e9, 0.25, 14, 0, True, ft)[2] == MR.MAX_GRID


def test_cases_hold_what_the_issue_asks():
    c = MC.case("base")
    use = MC.in_use(c)
    b = c["boxes"][use]
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    assert (b[:, 0] < 0).any() and (b[:, 1] < 0).any() and (b[:, 2] > MC.IMG).any() and (b[:, 3] > MC.IMG).any(), "outside on each side"
    assert ((w > MC.IMG) & (h > MC.IMG)).any() and (w == 0).any() and (np.maximum(w, h) / np.maximum(np.minimum(w, h), 1e-9) >= 8).any()
    assert np.ceil(np.clip(w, 0, MC.IMG) / MC.M).max() >= 3, "adaptive grid of at least 3 on the bitmaps"
    own = c["gt_boxes"]
    assert all((b == g).all(1).any() for g in own) and (own == np.round(own)).all(), "the gts' own integer boxes are among the positives"
    assert MC.case("odd")["C"] % 4 and MC.case("one_empty")["n_pos"].tolist()[1] == 0 and not MC.case("none")["n_pos"].any()
    for name in CASES:
        assert min(MC.margins(MC.case(name))) > MC.MARGIN and MC.level_margin(MC.case(name)) > 1e-3, name


def test_level_map_matches_the_extractor():
    ex = SingleRoIExtractor(dict(type="RoIAlign", output_size=14, sampling_ratio=0), 8, [4, 8, 16, 32], finest_scale=MC.FINEST)
    c = MC.case("base")
    rois = c["rois"][MC.in_use(c)]
    keep = (rois[:, 3] - rois[:, 1]) * (rois[:, 4] - rois[:, 2]) >= 0
    assert ex.map_roi_levels(torch.as_tensor(rois[keep]), 4).tolist() == MR.map_roi_levels(rois[keep], MC.FINEST, 4).tolist()
    assert ex.num_inputs == 4 and ex.geometry() == dict(out_size=14, sampling_ratio=0, aligned=True, finest_scale=MC.FINEST)


# ------------------------------------------------------------------------------------------------------------------- names, constructors, keys
def test_registry_names_and_state_dict(f25):
    for name, cls in (("RoIAlign", RoIAlign), ("mmcv.RoIAlign", RoIAlign), ("SingleRoIExtractor", SingleRoIExtractor), ("mmdet.SingleRoIExtractor", SingleRoIExtractor),
                      ("FCNMaskHead", FCNMaskHead), ("MTP_IS_FCNMaskHead", FCNMaskHead), ("MTP_IS_StandardRoIHead", MaskRoIHead)):
        assert MODELS.get(name) is cls, name
    assert MTP_IS_FCNMaskHead is FCNMaskHead and MTP_IS_StandardRoIHead is MaskRoIHead
    assert MODELS.get("StandardRoIHead") is not MaskRoIHead and MODELS.get("MTP_RD_StandardRoIHead") is not MaskRoIHead
    head = MODELS.build(head_cfg())
    assert sorted(head.state_dict()) == f25["base.state_keys"].tolist(), "the reference's state-dict keys"
    assert not any("conv_logits" in k for k in head.state_dict()) and head.with_mask and not head.with_bbox and head.slots == 8
    mh = head.mask_head
    assert mh.mask_size == 28 and mh.roi_feat_size == (14, 14) and mh.upsample_method == "deconv" and mh.scale_factor == 2 and not mh.class_agnostic
    for k, v in head.state_dict().items():
        assert tuple(v.shape) == tuple(MC.case("base")["weights"][k[len("mask_head."):]].shape), k
    plain = FCNMaskHead(num_convs=2, in_channels=8, conv_out_channels=16, upsample_cfg=dict(type=None))
    assert sorted(plain.state_dict()) == ["convs.%d.conv.%s" % (i, k) for i in (0, 1) for k in ("bias", "weight")] and plain.mask_size == 14
    full = FCNMaskHead()      # mask_rcnn.py: 4 convs, 256 channels, 14 -> 28
    assert full.num_convs == 4 and tuple(full.upsample.weight.shape) == (256, 256, 2, 2) and tuple(full.convs[0].conv.weight.shape) == (256, 256, 3, 3)
    layer = RoIAlign(output_size=(7, 7), spatial_scale=0.25, sampling_ratio=2, aligned=False)
    assert (layer.output_size, layer.spatial_scale, layer.sampling_ratio, layer.aligned, layer.pool_mode) == (7, 0.25, 2, False, "avg")


def test_refusals():
    for bad in ("carafe", "nearest", "bilinear"):
        with pytest.raises(NotImplementedError, match=bad):
            FCNMaskHead(upsample_cfg=dict(type=bad, scale_factor=2))
    with pytest.raises(ValueError):
        FCNMaskHead(upsample_cfg=dict(type="pixel_shuffle"))
    with pytest.raises(NotImplementedError, match="norm_cfg"):
        FCNMaskHead(norm_cfg=dict(type="BN"))
    with pytest.raises(NotImplementedError, match="conv_cfg"):
        FCNMaskHead(conv_cfg=dict(type="ConvWS"))
    with pytest.raises(NotImplementedError):
        FCNMaskHead(loss_mask=dict(type="CrossEntropyLoss", use_mask=False))
    with pytest.raises(NotImplementedError):
        FCNMaskHead(loss_mask=dict(type="DiceLoss"))
    with pytest.raises(NotImplementedError):
        FCNMaskHead(upsample_cfg=dict(type="deconv", scale_factor=4))
    with pytest.raises(ValueError):
        FCNMaskHead(init_cfg=dict(type="Normal"))
    with pytest.raises(ValueError):
        FCNMaskHead(conv_out_channels=12)
    with pytest.raises(ValueError):
        FCNMaskHead(precision="fp16")
    with pytest.raises(NotImplementedError, match="max"):
        RoIAlign(14, pool_mode="max")
    with pytest.raises(NotImplementedError, match="max"):
        roi_align(torch.zeros(1, 4, 8, 8), torch.zeros(1, 5), 7, pool_mode="max")
    with pytest.raises(NotImplementedError):
        RoIAlign((7, 14))
    with pytest.raises(ValueError):
        RoIAlign(ops.ROI_ALIGN_MAX_OUT + 1)
    with pytest.raises(ValueError):
        RoIAlign(14, sampling_ratio=-1)
    with pytest.raises(ValueError):
        roi_align(torch.zeros(1, 4, 8, 8), torch.zeros(1, 6), 7)
    ex = SingleRoIExtractor(dict(type="RoIAlign", output_size=14, sampling_ratio=0), 8, [4, 8, 16, 32])
    assert ex.finest_scale == 56.0
    with pytest.raises(NotImplementedError, match="roi_scale_factor"):
        ex([torch.zeros(1, 8, s, s) for s in (16, 8, 4, 2)], torch.zeros(1, 5), roi_scale_factor=1.2)
    with pytest.raises(NotImplementedError):
        SingleRoIExtractor(dict(type="RoIPool", output_size=7), 8, [4])
    with pytest.raises(ValueError):
        ex([torch.zeros(1, 8, 16, 16)], torch.zeros(1, 5))
    with pytest.raises(NotImplementedError, match="horizontal box half"):
        MODELS.build(head_cfg(bbox_head=dict(type="Shared2FCBBoxHead")))
    with pytest.raises(NotImplementedError, match="horizontal box half"):
        MODELS.build(head_cfg(bbox_roi_extractor=dict(type="SingleRoIExtractor")))
    with pytest.raises(NotImplementedError, match="share_roi_extractor"):
        MODELS.build(head_cfg(mask_roi_extractor=None))
    with pytest.raises(NotImplementedError, match="shared head"):
        MODELS.build(head_cfg(shared_head=dict(type="ResLayer")))
    with pytest.raises(TypeError):
        MODELS.build(head_cfg(mask_head=None))
    with pytest.raises(NotImplementedError, match="soft_mask_target"):
        MODELS.build(head_cfg(train_cfg=dict(mask_size=28, soft_mask_target=True)))
    with pytest.raises(ValueError):
        MODELS.build(head_cfg(train_cfg=dict(mask_size=14)))
    with pytest.raises(ValueError):      # the extractor's output is the head's input
        MODELS.build(head_cfg(mask_head=dict(type="FCNMaskHead", in_channels=16, conv_out_channels=8)))
    head = MODELS.build(head_cfg())
    with pytest.raises(NotImplementedError, match="soft_mask_target"):
        head.mask_head.get_targets([NS(pos_priors=torch.zeros(0, 4))], [NS(masks=torch.zeros(0, 4, 4))], dict(mask_size=28, soft_mask_target=True))
    with pytest.raises(NotImplementedError):
        head.test_mask_roi_feats([torch.zeros(1, 8, s, s) for s in (16, 8, 4, 2)], None, pos_inds=torch.zeros(1), bbox_feats=torch.zeros(1))
    with pytest.raises(ValueError):      # a conv_logits of the wrong width
        head.mask_head(torch.zeros(0, 8, 14, 14), torch.nn.Conv2d(16, 3, 1))
    # the oriented head keeps refusing a mask head (tests/test_roi_host.py pins the message)
    with pytest.raises(NotImplementedError, match="the mask branch is not built"):
        MODELS.get("StandardRoIHead")(bbox_roi_extractor=object(), bbox_head=object(), mask_head=dict(type="FCNMaskHead"))


# ------------------------------------------------------------------------------------------------------------------- empty inputs
def test_empty_inputs_never_touch_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded for an empty input")
    monkeypatch.setattr(ops, "lib", boom)
    x = torch.randn(2, 8, 16, 16, requires_grad=True)
    y = RoIAlign(14, 0.25)(x, torch.zeros(0, 5))
    assert tuple(y.shape) == (0, 8, 14, 14)
    y.sum().backward()
    assert tuple(x.grad.shape) == tuple(x.shape) and not x.grad.any()
    head = MODELS.build(head_cfg())
    feats = [torch.zeros(2, 8, s, s) for s in (16, 8, 4, 2)]
    assert tuple(head.mask_roi_extractor(feats, torch.zeros(0, 5)).shape) == (0, 8, 14, 14)
    conv_logits = torch.nn.Conv2d(8, 3, 1)
    assert tuple(head.mask_head(torch.zeros(0, 8, 14, 14)).shape) == (0, 8, 28, 28)
    assert tuple(head.mask_head(torch.zeros(0, 8, 14, 14), conv_logits).shape) == (0, 3, 28, 28)
    none = [NS(pos_priors=torch.zeros(0, 4), pos_assigned_gt_inds=torch.zeros(0, dtype=torch.int64), pos_gt_labels=torch.zeros(0, dtype=torch.int64))] * 2
    gts = [NS(masks=torch.zeros(0, 64, 64, dtype=torch.uint8))] * 2
    assert tuple(head.train_mask_forward(feats, none, None).shape) == (0, 8, 14, 14)
    out = head.mask_loss(dict(mask_preds=torch.zeros(0, 3, 28, 28)), none, gts)
    assert float(out["loss_mask"]["loss_mask"]) == 0.0 and tuple(out["mask_targets"].shape) == (0, 28, 28)
    assert tuple(head.mask_head.get_targets(none, gts, head.train_cfg).shape) == (0, 28, 28)
    results = [NS(bboxes=torch.zeros(0, 4), labels=torch.zeros(0, dtype=torch.int64)) for _ in range(2)]
    metas = [dict(ori_shape=(37, 53), scale_factor=(1.25, 0.8))] * 2
    assert tuple(head.test_mask_generate_rois(results).shape) == (0, 5)
    done = head.predict(feats, results, metas, conv_logits, rescale=False)
    assert all(tuple(r.masks.shape) == (0, 30, 66) and r.masks.dtype == torch.bool for r in done)
    head.test_cfg = dict(mask_thr_binary=-1)
    done = head.predict(feats, results, metas, conv_logits, rescale=True)
    assert all(tuple(r.masks.shape) == (0, 37, 53) and r.masks.dtype == torch.uint8 for r in done)


def test_wrappers_refuse_bad_arguments_before_the_library():
    z, boxes = torch.zeros(2, 3, 28, 28), torch.zeros(2, 4)
    sg, n_pos, bm = torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.mask_loss(z.double(), boxes, None, sg, n_pos, bm)
    with pytest.raises(ValueError):
        ops.mask_loss(z, boxes, None, torch.zeros(1, 3, dtype=torch.int64), n_pos, bm)
    with pytest.raises(TypeError):
        ops.mask_loss(z, boxes, None, sg, n_pos, bm.float())
    with pytest.raises(TypeError):
        ops.mask_loss(z, boxes, torch.zeros(2, dtype=torch.int32), sg, n_pos, bm)
    with pytest.raises(ValueError):
        ops.mask_paste(z, None, torch.zeros(3, 4), 8, 8)
    with pytest.raises(ValueError):
        ops.mask_paste(torch.zeros(0, 3, 28, 28), None, torch.zeros(0, 4), 8, 8)
    with pytest.raises(TypeError):
        ops.roi_align_fwd([], [(8, 8)], [0.25], 4, 1, torch.zeros(0, 5))
    with pytest.raises(ValueError):
        ops.roi_align_fwd([], [(8, 8)], [0.25], 4, 1, torch.zeros(1, 5), out_size=33)
    with pytest.raises(TypeError):
        ops.roi_align_bwd(torch.zeros(1, 3, 4), [], [(8, 8)], [0.25], 4, 1, torch.zeros(1, 5), out_size=2)
