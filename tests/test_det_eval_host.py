"""CPU: the references and input sets behind the DOTA-metric tests (tests/det_eval_ref.py, tests/det_eval_cases.py, fixture f24) and the host parts of
mtp_amd.evaluation.DOTAMetric.
  * det_eval_ref equals f24 (the reference's own metric.py run over stubs): tp / fp / counts exactly, recall / precision / AP / the metrics dict to
    1e-12; the fixture regenerates bit for bit where the reference is present;
  * every input set meets its conditions, its seed is the first that does, and the float32 IoU error on it stays below a quarter of the gap;
  * the recall quirk at num_gts = 10 (3 / 10, 6 / 10, 7 / 10 do not reach their point; 4 / 10 does), the image with only ignored gts, the VOC rule,
    the tie rule, the exact family (IoU exactly 0.5 in float32 and float64);
  * the Task1 text writer against the recorded files; rbox2qbox's corner order; a two-rank split through merge_ranks equals the single-rank result;
  * the constructor's and the wrappers' refusals that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

import box_cases as BC
import box_ref as BR
import det_eval_cases as C
import det_eval_ref as R
from conftest import GOLDEN
from mtp_amd import MODELS, DOTAMetric, ops
from mtp_amd.evaluation import rbox2qbox

sys.path.insert(0, GOLDEN)
from make_dota_metric import REF  # noqa: E402  (where the fixture's generator looks for the reference's metric.py)
CLASSES = ("plane", "ship", "storage-tank", "harbor")


# ------------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("mode", ["11points", "area"])
def test_restatement_equals_the_fixture(golden, mode):
    g = golden("f24_dota_metric.npz")
    det_results, annotations = C.case("fixture")
    tb = R.tables(det_results, annotations)
    for k, v in tb.items():
        assert np.array_equal(g["in." + k], v) and g["in." + k].dtype == v.dtype, k
    for thr in (0.5, 0.75):
        mean_ap, res = R.eval_rbbox_map(det_results, annotations, thr, mode == "11points")
        p = "%s.thr%02d." % (mode, int(thr * 100))
        assert abs(mean_ap - float(g[p + "mean_ap"])) < 1e-12
        for c, r in enumerate(res):
            q = "%scls%d." % (p, c)
            assert np.array_equal(np.hstack([t[0] for t in r["tpfp"]])[0], g[q + "tp"]) and np.array_equal(np.hstack([t[1] for t in r["tpfp"]])[0], g[q + "fp"])
            assert r["num_gts"] == int(g[q + "num_gts"]) and r["num_dets"] == int(g[q + "num_dets"])
            assert r["recall"].dtype == g[q + "recall"].dtype == np.float64 and r["precision"].dtype == g[q + "precision"].dtype == np.float32
            for key in ("recall", "precision", "ap"):
                assert np.abs(np.asarray(r[key], np.float64) - g[q + key]).max(initial=0.0) < 1e-12, (q, key)
    got = R.compute_metrics(det_results, annotations, [0.5, 0.75], mode == "11points")
    assert list(got.keys()) == g[mode + ".metrics.keys"].tolist() == ["mAP", "AP50", "AP75"]
    assert np.abs(np.array(list(got.values())) - g[mode + ".metrics.values"]).max() < 1e-12
    assert got["AP50"] > 0.3 > got["AP75"] > 0      # (a fixture in which something is found, and the thresholds tell apart)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference implementation is not on this machine")
def test_fixture_regenerates_bit_for_bit(golden, tmp_path):
    import make_dota_metric as M
    out = M.build()
    g = golden("f24_dota_metric.npz")
    assert sorted(out) == sorted(g)
    for k, v in out.items():
        v = np.asanyarray(v)
        assert v.dtype == g[k].dtype and v.shape == g[k].shape and v.tobytes() == g[k].tobytes(), k
    M.write_npz(str(tmp_path / "f24.npz"), out)
    assert open(tmp_path / "f24.npz", "rb").read() == open(os.path.join(GOLDEN, "f24_dota_metric.npz"), "rb").read()


# ------------------------------------------------------------------------------------------------------------------- input sets
@pytest.mark.parametrize("name", list(C.SPECS))
def test_case_conditions_and_first_seeds(name):
    assert BC.first_seed(lambda s: C.make(name, s), C.condition) == C.SEEDS[name]
    det_results, annotations = C.case(name)
    worst = 0.0
    for res, ann in zip(det_results, annotations):
        for k, d in enumerate(res):
            assert len(np.unique(d[:, 5])) == len(d) and np.array_equal(d, d.astype(np.float32))
            g = np.vstack([ann["bboxes"][ann["labels"] == k], ann["bboxes_ignore"][ann["labels_ignore"] == k]])
            if not len(d) or not len(g):
                continue
            assert min(d[:, 2:4].min(), g[:, 2:4].min()) >= C.MIN_SIDE
            iou = BR.box_iou_rotated(d[:, :5], g)
            assert np.abs(iou[..., None] - np.asarray(C.THRS)).min() > C.GAP
            if len(g) > 1:
                top = np.sort(iou, 1)[:, -2:]
                assert bool(((top[:, 1] - top[:, 0] >= C.GAP) | (top[:, 1] == 0)).all())
            worst = max(worst, float(np.abs(BR.box_iou_rotated(d[:, :5], g, dtype=BR.F32) - iou).max()))
    assert worst < C.GAP / 4, worst
    gts, K, D, nodet = C.SPECS[name]
    tb = R.tables(det_results, annotations)
    assert np.diff(tb["gt_start"]).tolist() == list(gts) and (D is None or len(tb["det_scores"]) == D)
    assert all(not (tb["det_img"] == i).any() for i in nodet)


def test_sets_cover_what_the_kernel_tests_claim():
    tb, _, best_gt, flags, num_gts = C.expected("fixture", (0.5, 0.75))
    assert (flags[0] == R.TP).sum() > 5 and (flags[0] == 0).sum() > 3 and (best_gt < 0).sum() > 3 and (flags[0] != flags[1]).any()
    img2 = tb["det_img"] == 2                      # the image with only ignored gts: no gts at all, every detection a false positive
    assert img2.sum() > 0 and (flags[:, img2] == R.FP).all() and (best_gt[img2] == -1).all()
    assert tb["gt_ignore"][tb["gt_start"][2]:tb["gt_start"][3]].all() and tb["gt_start"][3] - tb["gt_start"][2] == 3
    ig = tb["gt_ignore"][np.maximum(best_gt, 0)].astype(bool) & (best_gt >= 0)
    assert (ig & (flags[0] == 0)).sum() > 3 and (flags[0][ig & (C.expected("fixture", (0.5, 0.75))[1] < 0.5)] == R.FP).all()
    _, _, _, _, n15 = C.expected("dets_255", (0.5,))
    assert (n15 == 0).sum() == 1                   # a class without gts


# ------------------------------------------------------------------------------------------------------------------- the rules
def test_recall_points_are_numpys_arange():
    assert list(ops.DET_AP_POINTS) == np.arange(0, 1 + 1e-3, 0.1).tolist() and len(ops.DET_AP_POINTS) == 11
    assert ops.DET_AP_POINTS[3] == 0.30000000000000004 and ops.DET_AP_POINTS[6] == 0.6000000000000001 and ops.DET_AP_POINTS[7] == 0.7000000000000001


@pytest.mark.parametrize("hits,points", [(3, 3), (6, 6), (7, 7), (4, 5), (10, 11)])
def test_recall_quirk_at_ten_gts(hits, points):
    """a recall of exactly 3 / 10 (6 / 10, 7 / 10) does not reach 0.30000000000000004 (...): one point fewer than hits + 1; 4 / 10 reaches 0.4"""
    f = C.recall_quirk_flags(hits)
    order, start = np.arange(len(f)), np.array([0, len(f)])
    ap, last, rec, prec = R.ap_from_flags(f, order, start, np.array([10]))
    assert last[0] == hits / 10 and rec.dtype == np.float64 and prec.dtype == np.float32
    want = np.float32(0)
    for _ in range(points):
        want += np.float32(1)
    assert ap[0] == want / np.float32(11) and ap.dtype == np.float32


def test_image_with_only_ignored_gts_has_no_gts_at_all():
    ann = [C._ann([], [], [C.G0], [0])]
    dets = [[np.asarray([C.G0 + [0.9]], np.float64)]]
    tb, best_iou, best_gt, flags, num_gts = R.table_results(dets, ann, [0.5])
    assert flags.tolist() == [[R.FP]] and best_gt.tolist() == [-1] and num_gts.tolist() == [0]
    ann = [C._ann([[500.0, 500.0, 10.0, 10.0, 0.0]], [0], [C.G0], [0])]      # one non-ignored gt anywhere: the ignored one counts again
    tb, best_iou, best_gt, flags, num_gts = R.table_results(dets, ann, [0.5])
    assert flags.tolist() == [[0]] and best_gt.tolist() == [1] and best_iou[0] > 0.999 and num_gts.tolist() == [1]


def test_voc_rule_ties_and_the_exact_family():
    _, best_iou, best_gt, flags, _ = R.table_results(*C.voc_case(), [0.5])
    assert best_gt.tolist() == [0, 0] and flags.tolist() == [[R.TP, R.FP]]
    b = BR.box_iou_rotated(C.voc_case()[0][0][0][1:, :5], C.voc_case()[1][0]["bboxes"])
    assert b[0, 0] > b[0, 1] > 0.5               # the free gt b clears the threshold too
    _, best_iou, best_gt, flags, _ = R.table_results(*C.ties_case(), [0.5, 0.75])
    assert best_gt.tolist() == [0, 0, 0, 1, 1, 2, 0] and flags.tolist() == [[R.FP, R.TP, R.FP, R.FP, R.TP, 0, R.FP]] * 2
    assert np.abs(best_iou[:3] - [0.9, 0.8, 0.7]).max() < 1e-5
    for dtype in (BR.F64, BR.F32):
        _, best_iou, best_gt, flags, _ = R.table_results(*C.exact_case(), [0.5, 0.25], dtype=dtype)
        assert best_iou.tolist() == [0.5, 0.25] and flags.tolist() == [[R.TP, R.FP], [R.TP, R.TP]]


# ------------------------------------------------------------------------------------------------------------------- host parts of the metric
def merged_reference(golden):
    """the merge of the fixture's detections under the recorded patch ids, by box_ref.nms per (original image, class)"""
    from make_dota_metric import MERGE_IOU_THR, PATCH_IDS
    tb = R.tables(*C.case("fixture"))
    names, index, shift = [], [], []
    for pid in PATCH_IDS:
        name, _, xy = pid.split("__", 2)
        x, y = (int(v) for v in xy.split("___"))
        if name not in names:
            names.append(name)
        index.append(names.index(name)), shift.append((x, y))
    boxes = tb["det_boxes"].copy()
    boxes[:, :2] += np.asarray(shift, np.float32)[tb["det_img"]]
    orig = np.asarray(index)[tb["det_img"]]
    groups = orig * len(CLASSES) + tb["det_labels"]
    keep = BR.nms(boxes, tb["det_scores"], MERGE_IOU_THR, groups, rotated=True)
    return names, boxes, tb["det_scores"], tb["det_labels"], orig, groups, keep


def test_merge_set_is_clear_of_the_nms_threshold():
    from make_dota_metric import MERGE_IOU_THR
    names, boxes, scores, labels, orig, groups, keep = merged_reference(None)
    iou = BR.box_iou_rotated(boxes, boxes)
    same = (groups[:, None] == groups[None]) & ~np.eye(len(boxes), dtype=bool)
    assert np.abs(iou[same] - MERGE_IOU_THR).min() > C.GAP and 10 < len(keep) < len(boxes) and len(names) == 2


def test_task1_writer_matches_the_recorded_files(golden, tmp_path):
    g = golden("f24_dota_metric.npz")
    names, boxes, scores, labels, orig, groups, keep = merged_reference(g)
    zip_path = DOTAMetric.write_task1(str(tmp_path / "Task1"), CLASSES, names, orig[keep], labels[keep], boxes[keep], scores[keep])
    for c in CLASSES:
        assert open(tmp_path / "Task1" / ("Task1_%s.txt" % c), "rb").read() == g["merge.Task1_%s.txt" % c].tobytes(), c
    import zipfile
    assert zip_path == str(tmp_path / "Task1" / "Task1.zip") and sorted(zipfile.ZipFile(zip_path).namelist()) == sorted("Task1_%s.txt" % c for c in CLASSES)
    with pytest.raises(ValueError):
        DOTAMetric.write_task1(str(tmp_path / "Task1"), CLASSES, names, orig[keep], labels[keep], boxes[keep], scores[keep])      # the path exists now


def test_rbox2qbox_corner_order():
    q = rbox2qbox(torch.tensor([[10.0, 20.0, 8.0, 4.0, 0.0], [0.0, 0.0, 2.0, 2.0, np.pi / 2]], dtype=torch.float64)).numpy()
    assert np.allclose(q[0], [14, 22, 14, 18, 6, 18, 6, 22]) and np.allclose(q[1], [-1, 1, 1, 1, 1, -1, -1, -1])


def test_two_rank_split_equals_one_rank():
    det_results, annotations = C.case("gts_63_64_65")
    K, thrs = 5, [0.5, 0.75]
    tb, _, _, flags, num_gts = R.table_results(det_results, annotations, thrs)
    parts = []
    for lo, hi in ((0, 2), (2, 3)):          # rank 0: images 0 and 1, rank 1: image 2 -- each matches its own images
        t, _, _, f, n = R.table_results(det_results[lo:hi], annotations[lo:hi], thrs)
        parts.append(tuple(torch.from_numpy(a) for a in (t["det_scores"], t["det_labels"], f, n)))
    s, l, f, n = (a.numpy() for a in DOTAMetric.merge_ranks(parts))
    assert np.array_equal(s, tb["det_scores"]) and np.array_equal(l, tb["det_labels"]) and np.array_equal(f, flags) and np.array_equal(n, num_gts)
    order, start = R.sorted_segments(s, l, K)
    for t in range(2):
        for a, b in zip(R.ap_from_flags(f[t], order, start, n), R.ap_from_flags(flags[t], *R.sorted_segments(tb["det_scores"], tb["det_labels"], K), num_gts)):
            assert a.tobytes() == b.tobytes()


def test_table_reference_agrees_with_the_list_reference():
    """ap_from_flags over table_results (what the kernels are compared with) = eval_rbbox_map (what f24 pins)"""
    det_results, annotations = C.case("fixture")
    tb, _, _, flags, num_gts = C.expected("fixture", (0.5, 0.75))
    order, start = R.sorted_segments(tb["det_scores"], tb["det_labels"], 4)
    for t, thr in enumerate((0.5, 0.75)):
        for mode in ("11points", "area"):
            ap, last, rec, prec = R.ap_from_flags(flags[t], order, start, num_gts, mode)
            _, res = R.eval_rbbox_map(det_results, annotations, thr, mode == "11points")
            for k, r in enumerate(res):
                assert ap[k] == r["ap"] and np.array_equal(rec[start[k]:start[k + 1]], r["recall"]) and np.array_equal(prec[start[k]:start[k + 1]], r["precision"])
                assert r["num_gts"] == num_gts[k]


def test_refusals_without_a_device():
    for name in ("DOTAMetric", "MTP_RD_Metric", "mmrotate.DOTAMetric"):
        assert MODELS.get(name) is DOTAMetric
    with pytest.raises(KeyError, match="metric should be one of 'mAP', but got bbox."):
        DOTAMetric(metric="bbox", classes=CLASSES)
    with pytest.raises(NotImplementedError, match="qbox"):
        DOTAMetric(predict_box_type="qbox", classes=CLASSES)
    with pytest.raises(NotImplementedError, match="scale_ranges"):
        DOTAMetric(scale_ranges=[(0, 32)], classes=CLASSES)
    with pytest.raises(ValueError, match="thresholds"):
        DOTAMetric(iou_thrs=[0.1 * i for i in range(1, 10)], classes=CLASSES)
    with pytest.raises(RuntimeError, match="class names"):
        DOTAMetric().classes
    m = DOTAMetric(iou_thrs=[0.5, 0.75], classes=CLASSES, metric=["mAP"])
    assert m.iou_thrs == [0.5, 0.75] and m.use_07_metric and m.prefix == "dota" and DOTAMetric(0.5, dataset_meta=dict(classes=CLASSES)).iou_thrs == [0.5]
    with pytest.raises(RuntimeError, match="nothing processed"):
        m.compute_metrics()
    b, s, l = torch.zeros(3, 5), torch.zeros(3), torch.zeros(3, dtype=torch.int64)
    g, gl, gi, st = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.uint8), torch.tensor([0, 2])
    with pytest.raises(ValueError, match="thresholds"):
        ops.det_match(b, s, l, l, g, gl, gi, st, [0.5] * 9)
    with pytest.raises(TypeError, match="det_labels"):
        ops.det_match(b, s, l.int(), l, g, gl, gi, st, [0.5])
    with pytest.raises(TypeError, match="gt_ignore"):
        ops.det_match(b, s, l, l, g, gl, gi.bool(), st, [0.5])
    with pytest.raises(TypeError, match="boxes"):
        ops.det_match(b.double(), s, l, l, g, gl, gi, st, [0.5])
    with pytest.raises(ValueError, match="classes"):
        ops.det_tpfp(s, s, l, gl, gi, [0.5], torch.zeros(1, 2, dtype=torch.int64), ops.DET_MAX_CLASSES + 1)
    with pytest.raises(ValueError, match="mode"):
        ops.det_ap(torch.zeros(1, 3, dtype=torch.uint8), l, torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), "voc")
    with pytest.raises(RuntimeError, match="device tensors"):
        m.process(dict(bboxes=b, scores=s, labels=l), dict(bboxes=g, labels=gl))
