"""GPU: the COCO-style metric of csrc/coco_eval.hip through mtp_amd.ops (mask_pack, coco_iou, coco_match, coco_accumulate) and
mtp_amd.evaluation.CocoMetric / eval_coco, every buffer out of a guard.Arena (poisoned outputs, guards on both sides, frozen inputs, the wrappers' own
workspaces included).  The reference is tests/coco_eval_ref.py, the numpy restatement of COCOeval (unpinned: see its docstring); the inputs are those
of tests/coco_eval_cases.py, whose conditions tests/test_coco_eval_host.py asserts.

Every comparison is EXACT, and that is derived, not measured: words, areas, intersections, flags and counts are integers; the float64 IoU, recall,
precision and scores are the same correctly rounded IEEE operations (+, -, *, /, fmin, fmax, int -> double) in the same order on both sides, with
contraction off in the kernels and no fused operation in numpy's scalar arithmetic; the twelve statistics are host numpy on bit-equal arrays."""
import numpy as np
import pytest
import torch

import coco_eval_cases as C
import coco_eval_ref as R
import guard
from mtp_amd import CocoMetric, eval_coco, ops

pytestmark = pytest.mark.gpu
ARENA = None


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
    """an op INPUT on the device, frozen (the arena has no poison for bool: such a tensor is a view of guarded uint8 storage)"""
    t = torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype == torch.bool:
        return ARENA.frozen(ARENA.like(t, dtype=torch.uint8)).view(torch.bool)
    return ARENA.frozen(ARENA.like(t))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 9), (65, 8, 8), (3, 5, 13), (2, 64, 65), (65, 1, 63), (1, 1, 4097), (0, 8, 8)])
def test_mask_pack_words_areas_and_zero_tail(shape):
    rng = np.random.default_rng(2710 + shape[0] + shape[2])
    m = rng.random(shape) < 0.5
    if shape[0]:
        m[0] = True      # a full mask: the tail of its last word must still be zero
    words, areas = ops.mask_pack(dev(m))
    w_words, w_areas = R.mask_pack(m) if shape[0] else (np.zeros((0, 1), np.uint64), np.zeros(0, np.int64))
    assert same_bits(words.cpu().numpy().view(np.uint64), w_words) and same_bits(areas.cpu().numpy(), w_areas)
    hw, u8 = shape[1] * shape[2], dev(m.astype(np.uint8) * 3)      # uint8 input, any non-zero value counts
    assert hw % 64 == 0 or shape[0] == 0 or int(words[0, -1]) == (1 << (hw % 64)) - 1
    assert same_bits(ops.mask_pack(u8)[0].cpu().numpy(), words.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------- IoU
def iou_inputs(images, kind):
    ds, gs = np.cumsum([0] + [len(im["labels"]) for im in images]), np.cumsum([0] + [len(im["gt_labels"]) for im in images])
    labels, gl = np.concatenate([im["labels"] for im in images]), np.concatenate([im["gt_labels"] for im in images])
    crowd = np.concatenate([im["gt_ignore"] for im in images]).astype(np.uint8)
    if kind == "bbox":
        det, gt = dev(np.concatenate([im["bboxes"] for im in images])), dev(np.concatenate([im["gt_bboxes"] for im in images]))
    else:
        det = ops.mask_pack(dev(np.concatenate([im["masks"] for im in images])))
        gt = ops.mask_pack(dev(np.concatenate([im["gt_masks"] for im in images])))
    return det, dev(labels), gt, dev(gl), dev(crowd), ds.tolist(), gs.tolist()


def want_iou(images, kind, agnostic):
    ious, inters = [], []
    for im in images:
        same = np.ones((len(im["labels"]), len(im["gt_labels"])), bool) if agnostic else im["labels"][:, None] == im["gt_labels"][None, :]
        if kind == "bbox":
            v = R.bbox_iou([R.xyxy2xywh(b) for b in im["bboxes"]], [R.xyxy2xywh(b) for b in im["gt_bboxes"]], im["gt_ignore"])
            n = np.zeros(v.shape, np.int64)
        else:
            flat = lambda x: x.reshape(x.shape[0], x.shape[1] * x.shape[2])      # noqa: E731
            v, n = R.mask_iou(flat(im["masks"]), flat(im["gt_masks"]), im["gt_ignore"])
        ious.append(np.where(same, v, 0.0).reshape(-1)), inters.append(np.where(same, n, 0).reshape(-1))
    return np.concatenate(ious), np.concatenate(inters)


@pytest.mark.parametrize("name,kind", [("fixture", "bbox"), ("fixture", "segm"), ("dyadic", "bbox"), ("gts_130", "bbox"), ("gts_130", "segm"),
                                       ("gts_63_64_65", "segm"), ("dets_100", "bbox")])
@pytest.mark.parametrize("agnostic", [False, True])
def test_iou_blocks_are_bit_equal(name, kind, agnostic):
    images = C.case(name)[0]
    det, labels, gt, gl, crowd, ds, gs = iou_inputs(images, kind)
    iou, inter, out_start = ops.coco_iou(kind, det, labels, gt, gl, crowd, ds, gs, agnostic=agnostic)
    w_iou, w_inter = want_iou(images, kind, agnostic)
    assert out_start[-1] == len(w_iou) and (w_iou > 0).sum() > 0
    if kind == "segm":
        assert same_bits(inter.cpu().numpy(), w_inter)
    got = iou.cpu().numpy()
    bad = np.nonzero(got.view(np.int64) != w_iou.view(np.int64))[0]
    assert len(bad) == 0, (name, kind, len(bad), got[bad[:5]], w_iou[bad[:5]])


# ------------------------------------------------------------------------------------------------------------------- match and accumulate
def device_inputs(images, kind):
    segm = kind == "segm"
    preds = [dict(bboxes=dev(im["bboxes"]), scores=dev(im["scores"]), labels=dev(im["labels"]), **(dict(masks=dev(im["masks"])) if segm else {})) for im in images]
    gts = [dict(bboxes=dev(im["gt_bboxes"]), labels=dev(im["gt_labels"]), ignore_flag=dev(im["gt_ignore"]), **(dict(masks=dev(im["gt_masks"])) if segm else {}))
           for im in images]
    return preds, gts, [im["img_id"] for im in images]


def check_eval(images, kind, K, thrs, max_dets, tag):
    """flags, ranks, npig, precision, recall, scores and the statistics against the restatement, all exact"""
    E = R.evaluate(images, kind, K, thrs, max_dets)
    preds, gts, ids = device_inputs(images, kind)
    got = eval_coco(preds, gts, K, metric=kind, iou_thrs=thrs, proposal_nums=max_dets, img_ids=ids)
    score, cat, rank, matched, ignored, npig = got["parts"]
    w_m, w_g, w_rank, w_score, w_label, w_npig = R.list_flags(E)
    assert np.array_equal(rank, w_rank) and np.array_equal(score.astype(np.float64), w_score) and np.array_equal(cat, w_label), tag
    assert np.array_equal(npig, w_npig), (tag, npig, w_npig)
    assert np.array_equal(matched, w_m), (tag, np.argwhere(matched != w_m)[:10])
    assert np.array_equal(ignored, w_g), (tag, np.argwhere(ignored != w_g)[:10])
    for k in ("precision", "recall", "scores"):
        assert same_bits(got[k], E.eval[k]), (tag, k, np.argwhere(got[k] != E.eval[k])[:10])
    assert same_bits(got["stats"], E.stats), tag
    return got, E


@pytest.mark.parametrize("name,kind", [(n, k) for n in C.SPECS for k in ("bbox", "segm", "proposal") if k != "segm" or C.SPECS[n][2].get("masks")])
def test_generated_sets_equal_the_restatement(name, kind):
    images, K, max_dets = C.case(name)
    got, _ = check_eval(images, kind, K, None, max_dets, (name, kind))
    assert name == "gts_0_1" or (got["parts"][3] != 0).sum() > 0      # the set is not vacuous


@pytest.mark.parametrize("name", ["gts_63_64_65", "dets_5"])
def test_one_threshold(name):
    images, K, max_dets = C.case(name)
    check_eval(images, "bbox", K, [0.5], max_dets, (name, "T1"))


@pytest.mark.parametrize("name", list(C.HAND))
def test_hand_cases(name):
    images, kind, K, thrs, max_dets = C.HAND[name]()
    check_eval(images, kind, K, thrs, max_dets, name)


def test_accumulate_segments_and_chunk_carry():
    """category segments of 0, 1, 255, 256, 257 and 1000 list positions with random flags and ranks, against accumulate_segment per (k, a, m, t)"""
    seg, T, A, mds = (0, 1, 255, 256, 257, 1000), 3, ops.COCO_AREAS, (2, 10, 100)
    rng = np.random.default_rng(2720)
    cat = rng.permutation(np.repeat(np.arange(len(seg)), seg)).astype(np.int64)
    D, K = len(cat), len(seg)
    matched, ignored = rng.choice(np.array([0, 1], np.uint8), (A, T, D)), rng.choice(np.array([0, 0, 1], np.uint8), (A, T, D))
    rank = rng.choice(np.array([0, 1, 5, 9, 10, 50, 99, 100, 300], np.int32), D)
    score = (np.floor(rng.random(D) * 64) / 64).astype(np.float32)      # runs of equal scores: the stable order decides
    npig = rng.integers(1, 400, (K, A)).astype(np.int64)
    npig[3, 1] = 0
    s = dev(score)
    o1 = torch.sort(s, descending=True, stable=True)[1]
    sorted_cat, o2 = torch.sort(dev(cat)[o1], stable=True)
    start = torch.searchsorted(sorted_cat.contiguous(), torch.arange(K + 1, device="cuda")).contiguous()
    pr, sc, rc = ops.coco_accumulate(dev(matched), dev(ignored), dev(rank), s, ARENA.frozen(o1[o2].contiguous()), ARENA.frozen(start), dev(npig), mds)
    pr, sc, rc = pr.cpu().numpy(), sc.cpu().numpy(), rc.cpu().numpy()
    rec = np.array(ops.COCO_REC_POINTS)
    for k in range(K):
        for a in range(A):
            for m, md in enumerate(mds):
                keep = (cat == k) & (rank < md)
                if npig[k, a] == 0:
                    w = (-np.ones((T, 101)), -np.ones((T, 101)), -np.ones(T))
                else:
                    w = R.accumulate_segment(matched[a][:, keep] != 0, ignored[a][:, keep] != 0, score[keep].astype(np.float64), npig[k, a], rec)
                assert same_bits(pr[:, :, k, a, m], w[0]) and same_bits(sc[:, :, k, a, m], w[1]) and same_bits(rc[:, k, a, m], w[2]), (k, a, m)


# ------------------------------------------------------------------------------------------------------------------- the metric
def feed(metric, images, kinds_segm, which=None):
    """process under sync-debug 'error': any host synchronisation raises"""
    preds, gts, ids = device_inputs(images, "segm" if kinds_segm else "bbox")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for j in range(len(images)):
            if which is None or j in which:
                metric.process(preds[j], gts[j], ids[j])
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_metric_gives_f27_dicts_two_calls_and_the_one_sync(golden):
    """CocoMetric on f27's set gives the dict the reference's own compute_metrics returned (keys, order, values) and f27's arrays and statistics;
    two runs give the same bits; process makes no host sync and compute_metrics exactly one (counted under sync-debug 'warn')"""
    import warnings
    g = golden("f27_coco_metric.npz")
    images, K, max_dets = C.case("fixture")
    names = ["c%d" % k for k in range(K)]
    runs = []
    for _ in range(2):
        m = CocoMetric(metric=["bbox", "segm", "proposal"], classwise=True, classes=names)
        feed(m, images, True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                out = m.compute_metrics()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message) for w in seen) == 1, [str(w.message) for w in seen]
        runs.append((out, m.arrays))
    assert list(runs[0][0].keys()) == g["metrics.keys"].tolist() and list(runs[0][0].values()) == g["metrics.values"].tolist()
    for kind in ("bbox", "segm", "proposal"):
        for k in ("precision", "scores", "recall", "stats"):
            assert runs[0][1][kind][k].tobytes() == g["%s.%s" % (kind, k)].tobytes(), (kind, k)
            assert runs[0][1][kind][k].tobytes() == runs[1][1][kind][k].tobytes(), (kind, k)
    assert m.evaluate() == {"coco/" + k: v for k, v in runs[1][0].items()} and m.num_images == 0


def test_two_rank_split_through_gather():
    images, K, _ = C.case("fixture")
    names = ["c%d" % k for k in range(K)]
    one = CocoMetric(metric="segm", classes=names)
    feed(one, images, True)
    want = one.compute_metrics()
    r0, r1 = CocoMetric(metric="segm", classes=names), CocoMetric(metric="segm", classes=names)
    feed(r0, images, True, (0, 1, 2))
    feed(r1, images, True, (3, 4, 5))
    sent = []
    r1.gather = lambda part: (sent.append(part), [part])[1]
    r1.compute_metrics()
    r0.gather = lambda part: [part, sent[0]]
    assert r0.compute_metrics() == want and all(same_bits(r0.arrays["segm"][k], one.arrays["segm"][k]) for k in one.arrays["segm"])
    assert len(sent[0]) == 6      # only (score, category, rank, matched, ignored, npig) cross the ranks


def test_rank_without_images_takes_part_in_the_gather():
    images, K, _ = C.case("fixture")
    names = ["c%d" % k for k in range(K)]
    one, sent = CocoMetric(metric="segm", classes=names), []
    feed(one, images, True)
    one.gather = lambda part: (sent.append(part), [part])[1]
    want = one.compute_metrics()
    idle, mine = CocoMetric(metric="segm", classes=names), []
    idle.gather = lambda part: (mine.append(part), [sent[0], part])[1]
    assert idle.compute_metrics() == want and mine[0][0].numel() == 0 and tuple(mine[0][3].shape) == (4, 10, 0) and int(mine[0][5].sum()) == 0


def test_labels_outside_the_classes_are_left_out_and_their_entries_zeroed():
    images, K, max_dets = C.case("gts_0_1")
    preds, gts, ids = device_inputs(images, "bbox")
    want = eval_coco(preds, gts, K, img_ids=ids)
    stray = dict(bboxes=dev(np.array([[1, 1, 30, 30], [2, 2, 40, 40]], np.float32)), scores=dev(np.array([.99, .98], np.float32)), labels=dev(np.array([K, -1])))
    more = dict(preds[0], **{k: torch.cat([preds[0][k], stray[k]]) for k in stray})
    got = eval_coco([more] + preds[1:], gts, K, img_ids=ids)
    assert all(same_bits(got[k], want[k]) for k in ("precision", "scores", "recall", "stats"))
    score, cat, rank, matched, ignored, _ = got["parts"]
    assert cat[-2:].tolist() == [K, K] and rank[-2:].tolist() == [0, 0] and not matched[:, :, -2:].any() and not ignored[:, :, -2:].any()


def test_refusals_before_any_launch():
    with pytest.raises(NotImplementedError, match="proposal_fast"):
        CocoMetric(metric="proposal_fast")
    with pytest.raises(NotImplementedError, match="ann_file"):
        CocoMetric(ann_file="a.json")
    with pytest.raises(KeyError):
        CocoMetric(metric="keypoints")
    with pytest.raises(ValueError, match="thresholds"):
        CocoMetric(iou_thrs=[0.5] * 17)
    with pytest.raises(TypeError):
        ops.mask_pack(torch.zeros(2, 8, 8, device="cuda"))
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="offsets"):
        ops.coco_iou("bbox", torch.zeros(0, 4, device="cuda"), z, torch.zeros(0, 4, device="cuda"), z, z.to(torch.uint8), [0, 1], [0, 0])
    with pytest.raises(ValueError, match="maxDets"):
        ops.coco_accumulate(torch.zeros(4, 1, 0, dtype=torch.uint8, device="cuda"), None, None, None, None, None, torch.zeros(1, 4, dtype=torch.int64, device="cuda"),
                            (1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="gts in one image"):
        ops.coco_match(torch.zeros(0, dtype=torch.float64, device="cuda"), z, z.double(), z.new_zeros(2), z.new_zeros(4, 0), z, z.to(torch.uint8),
                       z.new_zeros(4, 0).to(torch.uint8), z.new_zeros(2), 1, [0.5], 100, max_cell_gts=4097)
