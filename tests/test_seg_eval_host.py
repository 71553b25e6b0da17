"""CPU: sliding-window inference and the IoU metric, host side.
  * the torch restatement the GPU tests compare against (tests/seg_eval_ref.py) equals the reference's own output, fixture f18: sliding-window logits and
    areas bit for bit, metrics to 1e-12 in float64 with NaN in the same places; IoUMetric.total_area_to_metrics and compute_metrics likewise;
  * the separable window counts the host hands the kernel equal the reference loop's count_mat;
  * what the constructors refuse, the registry build from a config dict, the two-rank reduce hook."""
import numpy as np
import pytest
import torch

import seg_eval_ref as R


def _same(a, b, tol=1e-12):
    a, b = torch.as_tensor(np.asarray(a)).double().reshape(-1), torch.as_tensor(np.asarray(b)).double().reshape(-1)
    assert a.shape == b.shape and torch.equal(a.isnan(), b.isnan())
    k = ~a.isnan()
    assert (a[k] - b[k]).abs().max().item() <= tol if k.any() else True


# ------------------------------------------------------------------------------------------------ the restatement against fixture f18
@pytest.mark.parametrize("tag", sorted(R.F18_GEOMS))
def test_torch_slide_restatement_equals_the_reference_fixture_f18(golden, tag):
    d = golden("f18_seg_eval.npz")
    img, crop, stride = R.F18_GEOMS[tag]
    x = torch.from_numpy(d["slide.%s.input" % tag]).double()
    w = torch.from_numpy(d["slide.weight"]).double()
    assert tuple(x.shape[2:]) == img
    seg, preds, count = R.torch_slide_inference(x, R.standin_encode_decode(w, crop), crop, stride, w.shape[0])
    assert torch.equal(seg, torch.from_numpy(d["slide.%s.seg_logits" % tag]))
    counts = set(count.unique().long().tolist())
    assert counts == ({1, 2, 3, 4, 6} if tag == "a" else {1, 2, 3, 4, 6, 9})
    # the same loop fed the low-resolution logits (what the GPU tests record per window) is the same function
    wins, _ = R.slide_windows(*img, crop, stride)
    low = [torch.nn.functional.conv2d(x[:, :, y1:y1 + crop[0], x1:x1 + crop[1]], w, stride=4) for y1, x1 in wins]
    assert torch.equal(R.torch_slide_from_lowres(low, crop, stride, *img)[0], seg)


def test_torch_areas_and_metrics_equal_the_reference_fixture_f18(golden):
    from mtp_amd import IoUMetric
    d = golden("f18_seg_eval.npz")
    K, tot = 5, torch.zeros(3, 5, dtype=torch.int64)
    for i in range(3):
        pred, lab = torch.from_numpy(d["metric.%d.pred" % i]), torch.from_numpy(d["metric.%d.label" % i])
        a = R.torch_areas(pred, lab, K)
        for row, name in zip(a, ("intersect", "pred_label", "label")):
            assert torch.equal(row, torch.from_numpy(d["metric.%d.area_%s" % (i, name)]))
        assert torch.equal(a[1] + a[2] - a[0], torch.from_numpy(d["metric.%d.area_union" % i]))      # union is derived, as IoUMetric does
        tot += a
    assert int(d["metric.2.area_label"].sum()) == 0 and int(d["metric.0.area_label"][4]) == 0 and int(tot[1, 4]) == 0
    for tname, a in (("all", tot), ("ignored", R.torch_areas(torch.from_numpy(d["metric.2.pred"]), torch.from_numpy(d["metric.2.label"]), K))):
        args = (a[0], a[1] + a[2] - a[0], a[1], a[2])
        for fam in R.FAMILIES:
            for nan, ntag in ((None, "nan"), (0, "zero")):
                ref = {k.rsplit(".", 1)[1]: v for k, v in d.items() if k.startswith("metric.%s.%s.%s." % (tname, "+".join(fam), ntag))}
                ours, prod = R.torch_metrics(*args, fam, nan), IoUMetric.total_area_to_metrics(*args, list(fam), nan, 1)
                assert list(ours) == list(prod) and sorted(ours) == sorted(ref) and len(ref) >= 3
                for k in ref:
                    _same(ours[k], ref[k])
                    _same(prod[k], ref[k])
    assert np.isnan(d["metric.all.mIoU.nan.IoU"][4]) and d["metric.all.mIoU.zero.IoU"][4] == 0 and np.isnan(d["metric.ignored.mIoU.nan.aAcc"])


def test_compute_metrics_rounds_like_the_reference(golden):
    """the summary dict: np.round(nanmean * 100, 2) under the reference's names; per-class arrays exposed; reset() clears"""
    from mtp_amd import IoUMetric
    d = golden("f18_seg_eval.npz")
    m = IoUMetric(5, iou_metrics=["mIoU", "mDice", "mFscore"])
    with pytest.raises(RuntimeError):
        m.compute_metrics()
    m.areas = sum(R.torch_areas(torch.from_numpy(d["metric.%d.pred" % i]), torch.from_numpy(d["metric.%d.label" % i]), 5) for i in range(3))
    out = m.compute_metrics()
    assert list(out) == ["aAcc", "mIoU", "mAcc", "mDice", "mFscore", "mPrecision", "mRecall"]
    pre = "metric.all.mIoU+mDice+mFscore.nan."
    for k, v in out.items():
        ref = d[pre + (k if k == "aAcc" else k[1:])]
        assert v == np.round(np.nanmean(ref) * 100, 2), k
    _same(m.per_class["IoU"], d[pre + "IoU"])
    assert "aAcc" not in m.per_class
    m.reset()
    assert m.areas is None and m.per_class is None
    with pytest.raises(KeyError):
        IoUMetric(5, iou_metrics=["mAP"])


# ------------------------------------------------------------------------------------------------ window arithmetic
SWEEP = [(32, 32, 32), (33, 32, 32), (64, 32, 32), (65, 32, 32), (56, 32, 24), (88, 48, 32), (50, 32, 12), (60, 32, 14), (1024, 512, 384), (512, 512, 384),
         (100, 64, 7), (97, 13, 5), (40, 40, 1), (41, 40, 1), (7, 3, 2)]


@pytest.mark.parametrize("size,crop,stride", SWEEP)
def test_separable_window_counts_equal_the_reference_count_mat(size, crop, stride):
    """cy[y] * cx[x] = count_mat[y, x]: each axis against the reference loop run with the other axis a single window, and a cross pairing"""
    from mtp_amd.segmentors.encoder_decoder import slide_origins, window_counts
    wins, count = R.slide_windows(size, crop, (crop, crop), (stride, stride))
    c = window_counts(size, crop, stride)
    assert c.dtype == torch.int32 and c.min().item() >= 1
    assert torch.equal(c.long(), count[:, 0])
    assert slide_origins(size, crop, stride) == [y for y, x in wins if x == 0]
    # crossed with another axis of the sweep
    s2, c2, t2 = SWEEP[(SWEEP.index((size, crop, stride)) + 3) % len(SWEEP)]
    if size * s2 <= 1 << 18:
        wins, count = R.slide_windows(size, s2, (crop, c2), (stride, t2))
        assert torch.equal(c.long()[:, None] * window_counts(s2, c2, t2).long()[None], count)
        assert wins == [(y, x) for y in slide_origins(size, crop, stride) for x in slide_origins(s2, c2, t2)]


def test_window_counts_on_the_fixture_geometries():
    from mtp_amd.segmentors.encoder_decoder import slide_origins, window_counts
    for (H, W), crop, stride in R.F18_GEOMS.values():
        _, count = R.slide_windows(H, W, crop, stride)
        assert torch.equal(window_counts(H, crop[0], stride[0]).long()[:, None] * window_counts(W, crop[1], stride[1]).long()[None], count)
    assert slide_origins(88, 48, 32) == [0, 32, 40] and slide_origins(1024, 512, 384) == [0, 384, 512]


# ------------------------------------------------------------------------------------------------ constructors, registry, reduce hook
BACKBONE = dict(type="ViT_Win_RVSA_V3_WSZ7", img_size=64, patch_size=8, embed_dim=128, depth=4, num_heads=2, interval=2, qkv_bias=True, use_abs_pos_emb=True,
                out_indices=[0, 1, 2, 3], precision="fp32")
HEAD = dict(type="UPerHead", in_channels=[128] * 4, channels=8, num_classes=5)
TEST_CFG = dict(mode="slide", stride=(384, 384), crop_size=(512, 512))


def test_registry_builds_the_segmentor_from_a_config_dict():
    import mtp_amd
    assert mtp_amd.MODELS.get("EncoderDecoder") is mtp_amd.EncoderDecoder
    m = mtp_amd.MODELS.build(dict(type="EncoderDecoder", backbone=BACKBONE, decode_head=HEAD, test_cfg=TEST_CFG))
    assert isinstance(m.backbone, mtp_amd.ViT_Win_RVSA_V3_WSZ7) and isinstance(m.decode_head, mtp_amd.UPerHead)
    assert (m.num_classes, m.out_channels, m.align_corners) == (5, 5, False) and m.test_cfg["mode"] == "slide"
    # modules instead of dicts; no test_cfg = whole mode
    m2 = mtp_amd.EncoderDecoder(m.backbone, m.decode_head)
    assert m2.decode_head is m.decode_head and m2.test_cfg is None


def test_constructor_refusals():
    import mtp_amd
    from mtp_amd import ops
    with pytest.raises(NotImplementedError):
        mtp_amd.EncoderDecoder(BACKBONE, HEAD, neck=dict(type="FPN"))
    with pytest.raises(NotImplementedError):
        mtp_amd.EncoderDecoder(BACKBONE, HEAD, auxiliary_head=dict(type="FCNHead"))
    with pytest.raises(ValueError):
        mtp_amd.EncoderDecoder(BACKBONE, dict(HEAD, num_classes=257))
    with pytest.raises(ValueError):
        mtp_amd.EncoderDecoder(BACKBONE, HEAD, test_cfg=dict(mode="slide"))
    with pytest.raises(ValueError):
        mtp_amd.EncoderDecoder(BACKBONE, HEAD, test_cfg=dict(mode="tile"))
    with pytest.raises(ValueError):
        mtp_amd.IoUMetric(257)
    assert mtp_amd.IoUMetric(256).num_classes == 256 == ops.SEG_MAX_CLASSES
    # an image smaller than the crop: refused before anything runs
    m = mtp_amd.EncoderDecoder(BACKBONE, HEAD, test_cfg=dict(mode="slide", stride=(32, 32), crop_size=(64, 64)))
    for shape in ((1, 3, 63, 128), (1, 3, 128, 48)):
        with pytest.raises(ValueError, match="smaller than"):
            m.slide_inference(torch.zeros(shape))
    with pytest.raises(ValueError):
        m.predict(torch.zeros(1, 3, 64, 64), metric=mtp_amd.IoUMetric(5))
    # a stride larger than the crop leaves pixels no window covers (the reference asserts count_mat != 0)
    gap = mtp_amd.EncoderDecoder(BACKBONE, HEAD, test_cfg=dict(mode="slide", stride=(80, 80), crop_size=(64, 64)))
    with pytest.raises(ValueError, match="no window"):
        gap.slide_inference(torch.zeros(1, 3, 200, 200))
    # the ops refuse K > 256 and out-of-range classes on the host side, before any launch
    with pytest.raises(ValueError):
        ops.seg_areas(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), 257, torch.zeros(3, 257, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.seg_areas(torch.full((4,), 5, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), 5, torch.zeros(3, 5, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.seg_areas(torch.zeros(4, dtype=torch.int64), torch.tensor([0, 1, 255, -1]), 5, torch.zeros(3, 5, dtype=torch.int64))


def test_new_entry_points_reject_too_many_classes_and_bad_windows():
    """argument checks of the C entries, before any launch: K > 256, a window outside the map, mismatched optional pairs"""
    from mtp_amd import _lib
    lib = _lib.load()
    buf = (_lib.C.c_float * 64)()
    p = _lib.C.cast(buf, _lib.C.c_void_p)
    assert lib.mtp_seg_argmax_areas(p, 260, 1, 1, 1, 257, None, None, 0, p, None, None, 0, 255, None, None) == -1
    assert lib.mtp_seg_areas(p, 1, p, 1, 4, 257, 255, p, None) == -1
    assert lib.mtp_seg_argmax_areas(p, 8, 1, 1, 1, 7, p, None, 0, p, None, None, 0, 255, None, None) == -1          # cy without cx
    assert lib.mtp_seg_argmax_areas(p, 8, 1, 1, 1, 7, None, None, 0, p, None, p, 1, 255, None, None) == -1          # labels without areas
    assert lib.mtp_seg_argmax_areas(p, 8, 1, 1, 1, 7, None, None, 0, None, None, None, 0, 255, None, None) == -1    # nothing to write
    assert lib.mtp_seg_argmax_areas(p, 4, 1, 1, 1, 7, None, None, 0, p, None, None, 0, 255, None, None) == -1       # pitch below the classes
    for y1, x1 in ((-1, 0), (0, -1), (3, 0), (0, 5)):                                                                # 2 x 4 window in a 4 x 8 map
        assert lib.mtp_seg_window_accumulate(p, 0, 8, 1, 1, 1, 7, p, 8, 4, 8, y1, x1, 2, 4, None) == -1
    assert lib.mtp_seg_window_accumulate(p, 0, 8, 1, 1, 1, 7, p, 8, 4, 8, 0, 0, 5, 4, None) == -1                    # crop larger than the map
    assert lib.mtp_seg_window_accumulate(p, 0, 4, 1, 1, 1, 7, p, 8, 4, 8, 0, 0, 2, 4, None) == -1                    # pitch below the classes


def test_reduce_hook_sums_the_areas_of_two_ranks(golden):
    from mtp_amd import IoUMetric
    d = golden("f18_seg_eval.npz")
    a = [R.torch_areas(torch.from_numpy(d["metric.%d.pred" % i]), torch.from_numpy(d["metric.%d.label" % i]), 5) for i in range(2)]
    ranks = [IoUMetric(5), IoUMetric(5)]
    for r, m in enumerate(ranks):
        m.areas = a[r].clone()
        m.reduce = lambda t, other=a[1 - r]: t + other
    whole = IoUMetric(5)
    whole.areas = a[0] + a[1]
    ref = whole.compute_metrics()
    for r, m in enumerate(ranks):
        assert m.compute_metrics() == ref
        assert torch.equal(m.areas, a[r])                   # the rank's own counters are untouched: compute_metrics can be called again
        I, U, P, L = m.total_areas()
        assert torch.equal(I, (a[0] + a[1])[0]) and torch.equal(U, (a[0] + a[1])[1] + (a[0] + a[1])[2] - (a[0] + a[1])[0])
