"""CPU: the numpy restatement of the COCO evaluation (tests/coco_eval_ref.py) on the inputs of tests/coco_eval_cases.py: the conditions of the
committed seeds, the hand-computed cases, the two-section form of the greedy rule against the sequential loop, and the bit-word packing."""
import numpy as np
import pytest

import coco_eval_cases as C
import coco_eval_ref as R


P1 = 1.0 / (1.0 + np.spacing(1))      # the precision of "all true positives": tp / (fp + tp + np.spacing(1))


def run(name):
    images, kind, K, thrs, max_dets = C.HAND[name]()
    E = R.evaluate(images, kind, K, thrs, max_dets)
    return E, R.list_flags(E)


def cell(E, k=0, a=0, i=0):
    p = E._paramsEval
    return E.evalImgs[k * len(p.areaRng) * len(p.imgIds) + a * len(p.imgIds) + i]


@pytest.mark.parametrize("name", list(C.SPECS))
def test_every_committed_seed_meets_the_conditions(name):
    images, K, _ = C.case(name)
    assert C.seed_ok(images)
    assert [[(int(((im["gt_labels"] == k).sum())), int((im["labels"] == k).sum())) for k in range(K)] for im in images] == C.SPECS[name][0]


def test_recall_points_and_area_ranges_are_cocoeval_s():
    from mtp_amd import ops
    p = R.Params()
    assert np.array_equal(np.array(ops.COCO_REC_POINTS), p.recThrs) and np.array_equal(np.array(ops.COCO_AREA_RNG), np.array(p.areaRng, np.float64))


def test_equal_iou_later_gt_wins():
    E, _ = run("equal_iou_later_wins")
    e = cell(E)
    assert E.ious[0, 0].tolist() == [[0.5, 0.5], [0.5, 0.5]] and e["dtMatches"].tolist() == [[2.0, 1.0]] and e["gtIds"] == [1, 2]


def test_non_ignored_gt_of_lower_iou_is_preferred():
    E, (m, g, *_ ) = run("non_ignored_before_ignored")
    e = cell(E)
    assert E.ious[0, 0].tolist() == [[1.0, 0.625]] and e["gtIds"] == [2, 1] and e["dtMatches"].tolist() == [[2.0]] and g[0].tolist() == [[0]]


def test_crowd_gt_is_matched_twice_and_both_are_ignored():
    E, (m, g, _, _, _, npig) = run("crowd_matched_twice")
    assert cell(E)["dtMatches"].tolist() == [[1.0, 1.0]] and m[0].tolist() == [[1, 1]] and g[0].tolist() == [[1, 1]] and npig.tolist() == [[1, 1, 0, 0]]
    assert E.eval["recall"][0, 0, 0, 2] == 0 and (E.eval["precision"][0, :, 0, 0, 2] == 0).all()


def test_unmatched_detection_is_ignored_only_outside_the_range():
    _, (m, g, *_ ) = run("unmatched_outside_range")
    assert m[:, 0, 0].tolist() == [0, 0, 0, 0] and g[:, 0, 0].tolist() == [0, 0, 1, 1]


def test_area_edges_count_in_both_ranges():
    _, (m, g, _, _, _, npig) = run("area_edges")
    assert npig.tolist() == [[1, 1, 1, 0], [1, 0, 1, 1]] and m[:, 0].tolist() == [[1, 1]] * 4 and g[:, 0].tolist() == [[0, 0], [0, 1], [0, 0], [1, 0]]


def test_mask_iou_of_exactly_one_half_matches_at_one_half():
    E, (m, *_ ) = run("mask_half")
    assert E.ious[0, 0].tolist() == [[0.5]] and m[0].tolist() == [[1]] and cell(E)["gtIds"] == [1]
    assert [d["area"] for d in E.cocoDt.dataset["annotations"]] == [2] and [g["area"] for g in E.cocoGt.dataset["annotations"]] == [4.0]      # pixels; the BOX


def test_iou_one_matches_at_threshold_one():
    E, (m, *_ ) = run("iou_one_at_one")
    assert E.ious[0, 0].tolist() == [[1.0]] and m[0].tolist() == [[1]] and E.stats[0] == np.mean(np.full(101, P1))


def test_recall_thresholds_past_the_last_recall_read_zero():
    E, _ = run("recall_past_the_end")
    pr = E.eval["precision"][0, :, 0, 0, 2]
    assert E.eval["recall"][0, 0, 0, 2] == 0.5 and (pr[:51] == P1).all() and (pr[51:] == 0.0).all() and E.stats[0] == np.mean(pr)


def test_no_counted_gt_leaves_minus_one():
    E, (_, _, _, _, _, npig) = run("no_counted_gt")
    assert npig[:, 0].tolist() == [0, 0, 1]
    for k in (0, 1):
        assert (E.eval["precision"][:, :, k] == -1).all() and (E.eval["recall"][:, k] == -1).all() and (E.eval["scores"][:, :, k] == -1).all()
    assert (E.eval["precision"][0, :, 2, 0, 2] == P1).all() and E.stats[0] == np.mean(np.full(101, P1))


def test_max_dets_prefix_is_per_cell():
    E, (_, _, rank, *_ ) = run("max_dets_per_cell")
    assert rank.tolist() == [0, 1, 0, 1] and E.eval["recall"][0, :, 0, 0].tolist() == [1.0, 1.0] and E.stats[6] == 1.0


def test_two_section_form_equals_the_sequential_loop():
    rng = np.random.default_rng(2730)
    for _ in range(3000):
        D, G = rng.integers(1, 6), rng.integers(1, 7)
        ious = rng.choice(np.array([0.0, 0.3, 0.5, 0.5, 0.6, 0.75, 0.9, 1.0]), (D, G))
        ig = np.sort(rng.integers(0, 2, G))
        crowd = (ig == 1) & (rng.random(G) < 0.5)
        thrs = [0.5, 0.75, 1.0]
        assert np.array_equal(R.match_sequential(ious, thrs, ig, crowd), R.match_two_sections(ious, thrs, ig, crowd))


def test_mask_pack_bit_order_and_tail():
    m = np.zeros((2, 1, 70), bool)
    m[0, 0, [0, 63, 64, 69]] = True
    words, areas = R.mask_pack(m)
    assert words.tolist() == [[(1 << 63) | 1, (1 << 5) | 1], [0, 0]] and areas.tolist() == [4, 0] and words.dtype == np.uint64
    enc = R.encode_masks(m)
    assert all(np.array_equal(R.decode_mask(e), x.reshape(-1)) for e, x in zip(enc, m))


# ---------------------------------------------------------------------------------------------------------------- fixture f27
F27_KINDS = ("bbox", "segm", "proposal")


def test_fixture_inputs_are_the_generated_set(golden):
    """f27's recorded inputs are case('fixture'): what the reference's metric.py was run on is what these tests run on"""
    from make_coco_metric import inputs
    g = golden("f27_coco_metric.npz")
    images = C.case("fixture")[0]
    assert int(g["seed"]) == C.SEEDS["fixture"]
    for k, v in inputs(images).items():
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k]), k


@pytest.mark.parametrize("kind", F27_KINDS)
def test_restatement_reproduces_f27(golden, kind):
    """the restatement driven by coco_eval_ref.to_coco / evaluate equals the restatement driven by the reference's own process, gt_to_coco_json,
    results2json and json files: conversions, parameters, flags, counts and every array, exactly"""
    g = golden("f27_coco_metric.npz")
    images, K, max_dets = C.case("fixture")
    E = R.evaluate(images, kind, K, None, max_dets)
    p = E._paramsEval
    assert str(g[kind + ".iouType"]) == p.iouType and int(g[kind + ".useCats"]) == p.useCats
    assert g[kind + ".imgIds"].tolist() == list(p.imgIds) and g[kind + ".catIds"].tolist() == list(p.catIds)
    assert g[kind + ".maxDets"].tolist() == list(p.maxDets) and np.array_equal(g[kind + ".iouThrs"], p.iouThrs)
    assert np.array_equal(g[kind + ".dt_area"], np.array([a["area"] for a in E.cocoDt.dataset["annotations"]], np.float64))
    assert np.array_equal(g[kind + ".gt_area"], np.array([a["area"] for a in E.cocoGt.dataset["annotations"]], np.float64))
    assert np.array_equal(g[kind + ".gt_bbox"], np.array([a["bbox"] for a in E.cocoGt.dataset["annotations"]], np.float64))
    if kind != "segm":
        assert np.array_equal(g[kind + ".dt_bbox"], np.array([a["bbox"] for a in E.cocoDt.dataset["annotations"]], np.float64))
    for k in ("precision", "recall", "scores"):
        assert E.eval[k].tobytes() == g["%s.%s" % (kind, k)].tobytes() and E.eval[k].shape == g["%s.%s" % (kind, k)].shape, k
    assert np.asarray(E.stats).tobytes() == g[kind + ".stats"].tobytes()
    for k, v in zip(("matched", "ignored", "rank", "score", "label", "npig"), R.list_flags(E)):
        assert v.dtype == g["%s.list.%s" % (kind, k)].dtype and np.array_equal(v, g["%s.list.%s" % (kind, k)]), k


def test_metrics_dict_equals_the_reference_s(golden):
    """key names, order and rounding of metric.py:493-580 (classwise entries included; 'segm' overwrites the '<name>_precision' of 'bbox' in place)"""
    g = golden("f27_coco_metric.npz")
    images, K, max_dets = C.case("fixture")
    want = {}
    for kind in F27_KINDS:
        E = R.evaluate(images, kind, K, None, max_dets)
        want.update(R.metrics_dict(E.stats, E.eval["precision"], kind, ["c%d" % k for k in range(K)], classwise=True))
    assert list(want) == g["metrics.keys"].tolist() and [want[k] for k in want] == g["metrics.values"].tolist()
