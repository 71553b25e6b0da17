"""GPU: the DOTA mAP metric of csrc/det_eval.hip through mtp_amd.ops (det_match, det_tpfp, det_ap) and mtp_amd.evaluation.DOTAMetric, every buffer out
of a guard.Arena (poisoned outputs, guards on both sides, frozen inputs, the wrappers' own workspaces included).  The reference is
tests/det_eval_ref.py (pinned by fixture f24, the reference's own metric.py); the inputs are those of tests/det_eval_cases.py, whose conditions
tests/test_det_eval_host.py asserts.
  * fixture f24 on the device: flags, counts, recall / precision arrays, 11-point AP exactly; compute_metrics equals the recorded dict;
  * match seams: 0, 1, 63, 64, 65, 130 gts per image; D in {1, 255, 256, 257}; an image without detections; a class without gts; an ignored gt as
    the best match; two and three detections on one gt; equal scores (the lower index wins); the exact family (IoU exactly 0.5 matches at 0.5);
  * AP seams: class segments of 0, 1, 255, 256, 257 and 1000 detections (the chunk carry), T = 1 and 3, the recall quirk at num_gts = 10, a class
    with num_gts = 0 left out of the mean;
  * bounds: flags, best_gt, counts, recall, precision and 11-point AP exact; best_iou within 4 x the float32 CPU error of box_ref against float64
    (floor 1e-6), the rule of test_hip_box_ops.check_iou; area-mode AP within 4 x the distance of the restatement with float32 precisions from
    the one with float64 precisions (floor 1e-6); the worst ratio is recorded;
  * two calls give the same bits; process runs under sync-debug 'error'; a two-rank split through `gather`; the merge path against box_ref.nms per
    group and the recorded Task1 files; the functional eval_rbbox_map; reserved entries are refused before any launch."""
import numpy as np
import pytest
import torch

import box_ref as BR
import det_eval_cases as C
import det_eval_ref as R
import guard
from conftest import record_parity
from mtp_amd import DOTAMetric, eval_rbbox_map, ops

pytestmark = pytest.mark.gpu
ARENA = None
CLASSES = ("plane", "ship", "storage-tank", "harbor")
TABLE = ("det_boxes", "det_scores", "det_labels", "det_img", "gt_boxes", "gt_labels", "gt_ignore", "gt_start")


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    global ARENA
    ARENA = a = guard.Arena("cuda")
    monkeypatch.setattr(ops, "_scratch", a.scratch)
    yield a
    ARENA = None
    torch.cuda.synchronize()
    try:
        a.check()
    finally:
        a.close()


def dev(a):
    """an op INPUT on the device, frozen"""
    return ARENA.frozen(ARENA.like(torch.as_tensor(a)))


def hip_match(tb, thrs, K):
    """det_match + det_tpfp on the tables of det_eval_ref.tables -> (best_iou, best_gt, flags, num_gts) as numpy"""
    t = {k: dev(tb[k]) for k in TABLE}
    best_iou, best_gt, winner = ops.det_match(*(t[k] for k in TABLE), thrs)
    flags, num_gts = ops.det_tpfp(t["det_scores"], best_iou, best_gt, t["gt_labels"], t["gt_ignore"], thrs, winner, K)
    assert best_iou.dtype == torch.float32 and best_gt.dtype == torch.int64 and flags.dtype == torch.uint8 and num_gts.dtype == torch.int64
    return tuple(x.cpu().numpy() for x in (best_iou, best_gt, flags, num_gts))


def check_match(got, want, iou32, tag):
    """flags, best_gt and counts exact; best_iou within 4 x the float32 CPU error of box_ref against float64, floor 1e-6"""
    (best_iou, best_gt, flags, num_gts), (_, w_iou, w_gt, w_flags, w_num) = got, want
    assert np.array_equal(best_gt, w_gt), (tag, np.nonzero(best_gt != w_gt)[0][:10])
    assert np.array_equal(flags, w_flags), (tag, np.argwhere(flags != w_flags)[:10])
    assert np.array_equal(num_gts, w_num), tag
    err = float(np.abs(best_iou.astype(np.float64) - w_iou).max(initial=0.0))
    e32 = float(np.abs(np.asarray(iou32, np.float64) - w_iou).max(initial=0.0))
    record_parity("det_eval", "best_iou_" + tag, err)
    record_parity("det_eval", "best_iou_box_ref_f32_cpu_" + tag, e32)
    assert err < max(4 * e32, 1e-6), (tag, err, e32)


def hip_ap(flags, scores, labels, num_gts, mode, curves=True):
    """the device sorts (stable by descending score, then stable by label) and det_ap -> numpy outputs and (order, cls_start)"""
    K = len(num_gts)
    s, l = dev(scores), dev(labels)
    o1 = torch.sort(s, descending=True, stable=True)[1]
    sl, o2 = torch.sort(l[o1], stable=True)
    order = o1[o2].contiguous()
    start = torch.searchsorted(sl, torch.arange(K + 1, device="cuda")).contiguous()
    out = ops.det_ap(dev(flags), ARENA.frozen(order), ARENA.frozen(start), dev(num_gts), mode, curves)
    return [None if x is None else x.cpu().numpy() for x in out], order.cpu().numpy(), start.cpu().numpy()


def check_ap(flags, scores, labels, num_gts, tag):
    """11 points: everything exact.  area: recall / precision exact, AP within 4 x |restatement(float32 precisions) - restatement(float64 precisions)|,
    floor 1e-6.  -> the worst area ratio"""
    T, K = flags.shape[0], len(num_gts)
    w_order, w_start = R.sorted_segments(scores, labels, K)
    worst = 0.0
    for mode in ("11points", "area"):
        (ap, num_dets, last, rec, prec), order, start = hip_ap(flags, scores, labels, num_gts, mode)
        assert np.array_equal(order, w_order) and np.array_equal(start, w_start) and np.array_equal(num_dets, np.diff(w_start)), (tag, mode)
        assert ap.dtype == np.float32 and ap.shape == last.shape == (T, K) and rec.dtype == np.float64 and prec.dtype == np.float32
        for t in range(T):
            w_ap, w_last, w_rec, w_prec = R.ap_from_flags(flags[t], w_order, w_start, num_gts, mode)
            assert np.array_equal(rec[t], w_rec) and np.array_equal(prec[t], w_prec) and np.array_equal(last[t], w_last), (tag, mode, t)
            if mode == "11points":
                assert np.array_equal(ap[t], w_ap), (tag, t, ap[t], w_ap)
            else:
                ap64 = R.ap_from_flags(flags[t], w_order, w_start, num_gts, mode, prec_dtype=np.float64)[0]
                for k in range(K):
                    bound = max(4 * abs(float(w_ap[k]) - float(ap64[k])), 1e-6)
                    err = abs(float(ap[t, k]) - float(ap64[k]))
                    worst = max(worst, err / bound)
                    assert err < bound, (tag, t, k, err, bound)
    record_parity("det_eval", "ap_area_worst_ratio_" + tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------- matching
@pytest.mark.parametrize("name", list(C.SPECS))
def test_match_and_flags_vs_reference(name):
    thrs = (0.5, 0.75) if name == "fixture" else (0.3, 0.5, 0.75)
    want = C.expected(name, thrs)
    K = C.SPECS[name][1]
    got = hip_match(want[0], list(thrs), K)
    iou32 = R.table_results(*C.case(name), [thrs[0]], dtype=BR.F32)[1]
    check_match(got, want, iou32, name)
    assert (got[2] == R.TP).sum() > 0 and ((got[2] == R.FP).sum() > 0 or name == "dets_1")


def test_fixture_flags_equal_the_recorded_ones(golden):
    """the reference's own tp / fp (per class, image order) against the device flags of the same detections"""
    g = golden("f24_dota_metric.npz")
    tb = {k: g["in." + k] for k in TABLE}
    best_iou, best_gt, flags, num_gts = hip_match(tb, [0.5, 0.75], 4)
    for t, thr in enumerate((50, 75)):
        for c in range(4):
            f = flags[t][tb["det_labels"] == c]          # table order inside a class = image order
            q = "11points.thr%02d.cls%d." % (thr, c)
            assert np.array_equal(f == R.TP, g[q + "tp"] > 0) and np.array_equal(f == R.FP, g[q + "fp"] > 0), q
            assert num_gts[c] == int(g[q + "num_gts"])


def test_ties_ignored_best_match_voc_rule_and_the_exact_family():
    for tag, case, thrs in (("ties", C.ties_case(), [0.5, 0.75]), ("voc", C.voc_case(), [0.5]), ("exact", C.exact_case(), [0.5, 0.25])):
        want = R.table_results(*case, thrs)
        got = hip_match(want[0], thrs, 1)
        check_match(got, want, R.table_results(*case, thrs[:1], dtype=BR.F32)[1], tag)
    assert got[0].tolist() == [0.5, 0.25] and got[2].tolist() == [[R.TP, R.FP], [R.TP, R.TP]]      # exactly 0.5 >= 0.5: a match
    ties = hip_match(R.tables(*C.ties_case()), [0.5], 1)
    assert ties[2].tolist() == [[R.FP, R.TP, R.FP, R.FP, R.TP, 0, R.FP]]      # rows 1 and 2 tie at 0.9: the lower index owns the gt; row 5: ignored gt


def test_no_gts_at_all():
    res, anns = C.case("gts_0_1")
    res, anns = res[:1], anns[:1]                 # the image without gts alone: G = 0
    want = R.table_results(res, anns, [0.5])
    assert len(want[0]["gt_labels"]) == 0 and len(want[0]["det_scores"]) > 0
    got = hip_match(want[0], [0.5], 3)
    assert (got[2] == R.FP).all() and (got[1] == -1).all() and (got[0] == 0).all() and got[3].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------- AP
SEGMENTS = (0, 1, 255, 256, 257, 1000)


def ap_set(T, seed):
    """class k holds SEGMENTS[k] detections (shuffled through the table); class 2 has no gts and no true positives"""
    rng = np.random.default_rng(24500 + seed)
    labels = rng.permutation(np.repeat(np.arange(len(SEGMENTS)), SEGMENTS)).astype(np.int64)
    D = len(labels)
    flags = rng.choice(np.array([0, 1, 1, 2, 2, 2], np.uint8), (T, D))
    flags[:, labels == 2] = np.where(flags[:, labels == 2] == R.TP, R.FP, flags[:, labels == 2])
    scores = ((rng.permutation(D) + 1.0) / (D + 1.0)).astype(np.float32)
    num_gts = np.array([max(int((flags[:, labels == k] == R.TP).sum(1).max(initial=0)), 0) + 3 for k in range(len(SEGMENTS))], np.int64)
    num_gts[2] = 0
    num_gts[4] = int((flags[:, labels == 4] == R.TP).sum(1).max())      # a class whose recall reaches exactly 1
    return flags, scores, labels, num_gts


@pytest.mark.parametrize("T", [1, 3])
def test_ap_segments_and_chunk_carry(T):
    flags, scores, labels, num_gts = ap_set(T, T)
    check_ap(flags, scores, labels, num_gts, "segments_T%d" % T)


def test_ap_equal_scores_keep_table_order():
    flags, scores, labels, num_gts = ap_set(1, 7)
    scores = np.round(scores * 8).astype(np.float32) / 8          # nine distinct values: long runs of equal scores
    check_ap(flags, scores, labels, num_gts, "equal_scores")


def test_ap_recall_quirk_on_the_device():
    hits = (3, 6, 7, 4)
    flags = np.concatenate([C.recall_quirk_flags(h) for h in hits])[None]
    labels = np.concatenate([np.full(h + 5, k, np.int64) for k, h in enumerate(hits)])
    scores = np.concatenate([np.linspace(0.9, 0.1, h + 5) for h in hits]).astype(np.float32)
    num_gts = np.full(4, 10, np.int64)
    (ap, _, last, _, _), _, _ = hip_ap(flags, scores, labels, num_gts, "11points")
    f11 = lambda n: np.float32(n) / np.float32(11)      # noqa: E731
    assert ap[0].tolist() == [f11(3), f11(6), f11(7), f11(5)] and last[0].tolist() == [0.3, 0.6, 0.7, 0.4]
    check_ap(flags, scores, labels, num_gts, "recall_quirk")


def test_two_calls_give_the_same_bits():
    want = C.expected("gts_130", (0.3, 0.5, 0.75))
    a, b = hip_match(want[0], [0.3, 0.5, 0.75], 5), hip_match(want[0], [0.3, 0.5, 0.75], 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    flags, scores, labels, num_gts = ap_set(3, 9)
    for mode in ("11points", "area"):
        (a, _, _), (b, _, _) = hip_ap(flags, scores, labels, num_gts, mode), hip_ap(flags, scores, labels, num_gts, mode)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), mode


# ------------------------------------------------------------------------------------------------------------------- the metric
def image_inputs(name, images=None):
    """per image: (pred dict, gt dict, ignored dict) of device tensors"""
    res, anns = C.case(name)
    out = []
    for i, (r, ann) in enumerate(zip(res, anns)):
        if images is not None and i not in images:
            continue
        d = np.vstack(r).astype(np.float32)
        labels = np.concatenate([np.full(len(x), k, np.int64) for k, x in enumerate(r)])
        out.append((dict(bboxes=dev(d[:, :5].copy()), scores=dev(d[:, 5].copy()), labels=dev(labels)),
                    dict(bboxes=dev(ann["bboxes"].astype(np.float32)), labels=dev(ann["labels"])),
                    dict(bboxes=dev(ann["bboxes_ignore"].astype(np.float32)), labels=dev(ann["labels_ignore"]))))
    return out


def feed(metric, inputs, ids=None):
    """process under sync-debug 'error': any host synchronisation raises"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for j, (p, g, ig) in enumerate(inputs):
            metric.process(p, g, ig, None if ids is None else ids[j])
        metric.tables()
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("mode", ["11points", "area"])
def test_metric_equals_the_fixture_dict(golden, mode):
    g = golden("f24_dota_metric.npz")
    m = DOTAMetric(iou_thrs=[0.5, 0.75], eval_mode=mode, dataset_meta=dict(classes=CLASSES))
    feed(m, image_inputs("fixture"))
    got = m.compute_metrics()
    keys, vals = g[mode + ".metrics.keys"].tolist(), g[mode + ".metrics.values"]
    assert list(got.keys()) == keys == ["mAP", "AP50", "AP75"]
    if mode == "11points":
        assert [got[k] for k in keys] == vals.tolist()
    else:
        assert abs(got["mAP"] - vals[0]) < 1e-6 and abs(got["AP50"] - vals[1]) <= 1e-3 and abs(got["AP75"] - vals[2]) <= 1e-3
    pc = m.per_class
    for t, thr in enumerate((50, 75)):
        for c in range(4):
            q = "%s.thr%02d.cls%d." % (mode, thr, c)
            assert pc["num_gts"][c] == int(g[q + "num_gts"]) and pc["num_dets"][c] == int(g[q + "num_dets"])
            assert pc["recall"][t, c] == (g[q + "recall"][-1] if len(g[q + "recall"]) else 0.0)
            assert pc["ap"][t, c] == g[q + "ap"] if mode == "11points" else abs(float(pc["ap"][t, c]) - float(g[q + "ap"])) < 1e-6
    assert m.evaluate() == {"dota/" + k: v for k, v in got.items()} and m.num_images == 0


def test_metric_reference_samples_and_a_class_without_gts():
    """the reference's call process(data_batch, data_samples); dets_255 has a class without gts, which the mean leaves out"""
    class Sample:
        def __init__(self, i, p, g, ig):
            self.img_id, self.r_pred_instances, self.r_gt_instances, self.r_ignored_instances = i, p, g, ig
    names = tuple("c%d" % k for k in range(15))
    m = DOTAMetric(iou_thrs=[0.5, 0.75], classes=names)
    m.process(None, [Sample(i, *x) for i, x in enumerate(image_inputs("dets_255"))])
    got = m.compute_metrics()
    want = R.compute_metrics(*C.case("dets_255"), [0.5, 0.75])
    assert got == want and m.per_class["num_gts"][10] == 0 and (m.per_class["num_gts"] > 0).sum() == 14
    mean = np.array([a for a, n in zip(m.per_class["ap"][0], m.per_class["num_gts"]) if n > 0]).mean().item()
    assert got["AP50"] == round(mean, 3) and mean != float(m.per_class["ap"][0].mean())


def test_two_rank_split_through_gather():
    one = DOTAMetric(iou_thrs=[0.5, 0.75], classes=CLASSES[:1] * 5)
    feed(one, image_inputs("gts_63_64_65"))
    want = one.compute_metrics()
    r0, r1 = DOTAMetric(iou_thrs=[0.5, 0.75], classes=CLASSES[:1] * 5), DOTAMetric(iou_thrs=[0.5, 0.75], classes=CLASSES[:1] * 5)
    feed(r0, image_inputs("gts_63_64_65", (0, 1)))
    feed(r1, image_inputs("gts_63_64_65", (2,)))
    sent = []
    r1.gather = lambda part: (sent.append(part), [part])[1]
    r1.compute_metrics()
    r0.gather = lambda part: [part, sent[0]]
    assert r0.compute_metrics() == want and all(np.array_equal(r0.per_class[k], one.per_class[k]) for k in one.per_class)
    assert len(sent[0]) == 4 and sent[0][2].shape[0] == 2      # only (scores, labels, flags, num_gts) cross the ranks


def test_functional_eval_rbbox_map():
    det_results, annotations = C.case("fixture")
    for use07 in (True, False):
        mean_ap, res = eval_rbbox_map(det_results, annotations, iou_thr=0.5, use_07_metric=use07)
        w_mean, w_res = R.eval_rbbox_map(det_results, annotations, 0.5, use07)
        for r, w in zip(res, w_res):
            assert r["num_gts"] == w["num_gts"] and r["num_dets"] == w["num_dets"]
            assert np.array_equal(r["recall"], w["recall"]) and np.array_equal(r["precision"], w["precision"]) and r["precision"].dtype == np.float32
            assert r["ap"] == w["ap"] if use07 else abs(float(r["ap"]) - float(w["ap"])) < 1e-6
        assert mean_ap == w_mean if use07 else abs(mean_ap - w_mean) < 1e-6


def test_merge_path_equals_box_ref_nms_per_group(golden, tmp_path):
    from make_dota_metric import MERGE_IOU_THR, PATCH_IDS
    from test_det_eval_host import merged_reference
    g = golden("f24_dota_metric.npz")
    names, boxes, scores, labels, orig, groups, keep = merged_reference(g)
    m = DOTAMetric(merge_patches=True, iou_thr=MERGE_IOU_THR, outfile_prefix=str(tmp_path / "Task1"), classes=CLASSES)
    feed(m, image_inputs("fixture"), PATCH_IDS)
    got = m.merged_detections()
    assert got[0] == names and np.array_equal(got[1], orig[keep]) and np.array_equal(got[2], labels[keep])
    assert np.array_equal(got[3], boxes[keep]) and np.array_equal(got[4], scores[keep])
    assert m.compute_metrics() == {}
    for c in CLASSES:
        assert open(tmp_path / "Task1" / ("Task1_%s.txt" % c), "rb").read() == g["merge.Task1_%s.txt" % c].tobytes(), c


def test_reserved_entries_are_refused_before_any_launch():
    tb = {k: dev(v) for k, v in C.expected("gts_0_1", (0.3, 0.5, 0.75))[0].items()}
    args = [tb[k] for k in TABLE]
    with pytest.raises(ValueError, match="thresholds"):
        ops.det_match(*args, [0.5] * 9)
    for i, k in enumerate(TABLE):
        bad = list(args)
        bad[i] = bad[i].to(torch.float64 if bad[i].dtype == torch.float32 else torch.int32)
        with pytest.raises(TypeError):
            ops.det_match(*bad, [0.5])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.det_match(args[0].repeat(1, 2)[:, :5], *args[1:], [0.5])
    with pytest.raises(NotImplementedError):
        DOTAMetric(predict_box_type="qbox", classes=CLASSES)
    with pytest.raises(NotImplementedError):
        DOTAMetric(scale_ranges=[(0, 32)], classes=CLASSES)
    with pytest.raises(NotImplementedError):
        eval_rbbox_map(*C.case("dets_1"), scale_ranges=[(0, 32)])
    with pytest.raises(ValueError, match="thresholds"):
        ops.det_ap(torch.zeros(9, 1, dtype=torch.uint8, device="cuda"), tb["det_labels"], tb["gt_start"][:2], tb["det_labels"])
