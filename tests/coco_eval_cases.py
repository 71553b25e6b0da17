"""Inputs of the COCO metric tests (host: tests/test_coco_eval_host.py, device: tests/test_hip_coco_eval.py, fixture f27: tests/golden/
make_coco_metric.py).  An image is a dict: img_id, height, width, bboxes (D, 4) float32 x1 y1 x2 y2, scores (D) float32, labels (D) int64, masks
(D, H, W) bool or None, gt_bboxes (G, 4) float32, gt_labels (G) int64, gt_ignore (G) uint8 (the reference's ignore_flag = iscrowd), gt_masks
(G, H, W) bool or None.

Generated sets: SPECS[name] = (images, classes, kwargs); every image is a list over the classes of (gts, detections) of that (image, category) cell.
SEEDS[name] is committed and `seed_ok` holds for each of them (asserted by the host test; no seed is skipped at run time): no box IoU within 1e-9
of a threshold of ALL_THRS without being equal to it, and no two IoUs of one detection within 1e-9 of each other unless they are equal -- so that no comparison the matching
makes hangs on the last bits of a quotient.  Mask IoUs are quotients of small integers and need no such care.

Hand cases: HAND[name]() -> (images, kind, classes, iou_thrs, max_dets); what each must give is asserted in the host test."""
import numpy as np

H, W = 120, 150      # 18000 pixels: 281 full words and a tail of 16
ALL_THRS = tuple(np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True).tolist()) + (0.3, 1.0)

# name -> (images: per image a list over the classes of (gts, dets), number of classes, options)
SPECS = {
    "fixture": ([[(3, 5), (0, 2), (2, 0)], [(0, 0), (0, 0), (0, 0)], [(4, 7), (2, 3), (1, 1)], [(0, 3), (3, 0), (2, 4)], [(5, 6), (1, 2), (0, 0)],
                 [(2, 2), (2, 2), (2, 2)]], 3, dict(masks=True)),
    "gts_0_1": ([[(0, 4), (1, 4)], [(1, 0), (0, 0)]], 2, dict(masks=True)),
    "gts_63_64_65": ([[(63, 20)], [(64, 20)], [(65, 20)]], 1, dict(masks=True)),
    "gts_130": ([[(130, 40), (3, 5)]], 2, dict(masks=True)),
    "dets_5": ([[(3, 0), (3, 1), (3, 4), (3, 5), (3, 6)], [(2, 6), (2, 5), (2, 4), (0, 1), (2, 0)]], 5, dict(masks=True)),
    "dets_100": ([[(12, 99), (12, 100), (12, 101)]], 3, dict()),
    "equal_scores": ([[(6, 30), (5, 25)], [(7, 30), (4, 20)]], 2, dict(levels=4, masks=True)),
    "dyadic": ([[(6, 12), (5, 9)], [(4, 10), (6, 8)]], 2, dict(dyadic=True)),
}
MAX_DETS = {"dets_5": (1, 3, 5), "dets_100": (2, 10, 100)}      # every other set: (100, 300, 1000)
SEEDS = {"fixture": 2700, "gts_0_1": 2701, "gts_63_64_65": 2702, "gts_130": 2703, "dets_5": 2704, "dets_100": 2705, "equal_scores": 2706, "dyadic": 2707}


def _box(rng, dyadic):
    """a box inside the image whose area falls in the small, medium or large range with equal chance"""
    lo, hi = ((4, 30), (34, 90), (98, 118))[rng.integers(3)]
    w, h = rng.uniform(lo, hi), rng.uniform(lo, min(hi, H - 2))
    x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
    b = np.array([x, y, x + w, y + h])
    return (np.round(b * 4) / 4 if dyadic else b).astype(np.float32)


def _mask(rng, box):
    """the box's pixels, with a little noise on them"""
    m = np.zeros((H, W), bool)
    x1, y1, x2, y2 = (int(round(float(v))) for v in box)
    m[max(y1, 0):max(y2, y1 + 1), max(x1, 0):max(x2, x1 + 1)] = True
    return m ^ (rng.random((H, W)) < 0.01)


def make_image(rng, cells, img_id, masks=False, dyadic=False, levels=0):
    gb, gl, db, dl = [], [], [], []
    for k, (ng, nd) in enumerate(cells):
        mine = [_box(rng, dyadic) for _ in range(ng)]
        gb += mine
        gl += [k] * ng
        for _ in range(nd):
            if mine and rng.random() < 0.75:      # a jittered copy of a gt of the class
                b = mine[rng.integers(ng)].astype(np.float64) + rng.normal(0, 3, 4)
                b[2:] = np.maximum(b[2:], b[:2] + 1)
                b = (np.round(b * 4) / 4 if dyadic else b).astype(np.float32)
            else:
                b = _box(rng, dyadic)
            db.append(b)
            dl.append(k)
    G, D = len(gb), len(db)
    perm = rng.permutation(D)      # the detections of the classes interleaved, as a detector's output is
    db, dl = [db[i] for i in perm], [dl[i] for i in perm]
    scores = rng.random(D).astype(np.float32)
    if levels:
        scores = (np.floor(scores * levels) / levels).astype(np.float32)      # long runs of equal scores
    arr = lambda rows: np.stack(rows).astype(np.float32) if rows else np.zeros((0, 4), np.float32)      # noqa: E731
    im = dict(img_id=img_id, height=H, width=W, bboxes=arr(db), scores=scores, labels=np.array(dl, np.int64), masks=None, gt_bboxes=arr(gb),
              gt_labels=np.array(gl, np.int64), gt_ignore=(rng.random(G) < 0.15).astype(np.uint8), gt_masks=None)
    if masks:
        stack = lambda boxes: np.stack([_mask(rng, b) for b in boxes]) if len(boxes) else np.zeros((0, H, W), bool)      # noqa: E731
        im["masks"], im["gt_masks"] = stack(db), stack(gb)
    return im


def build(name, seed):
    images, _, opts = SPECS[name]
    rng = np.random.default_rng(seed)
    return [make_image(rng, cells, i, **opts) for i, cells in enumerate(images)]


_CACHE = {}


def case(name):
    """-> (images, classes, max_dets); built once and shared: do not modify"""
    if name not in _CACHE:
        _CACHE[name] = (build(name, SEEDS[name]), SPECS[name][1], MAX_DETS.get(name, (100, 300, 1000)))
    return _CACHE[name]


def seed_ok(images, thrs=ALL_THRS, tol=1e-9):
    """the box condition of the module docstring, over every (detection, gt) pair of an image whatever the labels"""
    import coco_eval_ref as R
    for im in images:
        if not len(im["bboxes"]) or not len(im["gt_bboxes"]):
            continue
        d = [R.xyxy2xywh(b) for b in im["bboxes"]]
        g = [R.xyxy2xywh(b) for b in im["gt_bboxes"]]
        for crowd in (0, 1):
            iou = R.bbox_iou(d, g, [crowd] * len(g))
            near = iou[:, :, None] - np.asarray(thrs)[None, None, :]
            if ((np.abs(near) < tol) & (near != 0)).any():
                return False
            s = np.sort(iou, axis=1)
            gap = np.diff(s, axis=1)
            if ((gap < tol) & (gap != 0)).any():
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------- hand cases
def _img(img_id, dets, gts, masks=None, gt_masks=None, height=H, width=W):
    """dets: (x1, y1, x2, y2, score, label) rows; gts: (x1, y1, x2, y2, label, crowd) rows"""
    d, g = np.asarray(dets, np.float64).reshape(-1, 6), np.asarray(gts, np.float64).reshape(-1, 6)
    return dict(img_id=img_id, height=height, width=width, bboxes=d[:, :4].astype(np.float32), scores=d[:, 4].astype(np.float32),
                labels=d[:, 5].astype(np.int64), masks=masks, gt_bboxes=g[:, :4].astype(np.float32), gt_labels=g[:, 4].astype(np.int64),
                gt_ignore=g[:, 5].astype(np.uint8), gt_masks=gt_masks)


def _pixels(h, w, *sets):
    m = np.zeros((len(sets), h, w), bool)
    for i, s in enumerate(sets):
        for (y, x) in s:
            m[i, y, x] = True
    return m


DEFAULT = (100, 300, 1000)


def equal_iou_later_wins():
    """two gts with IoU exactly 1/2 with the first detection: it takes the LATER one; the second detection takes the other"""
    return [_img(0, [(0, 0, 10, 10, .9, 0), (0, 0, 10, 10, .8, 0)], [(0, 0, 10, 20, 0, 0), (0, 0, 20, 10, 0, 0)])], "bbox", 1, [0.5], DEFAULT


def non_ignored_before_ignored():
    """a crowd gt with IoU 1 (intersection over the detection's area) and a plain gt with IoU 0.625: the plain one is taken"""
    return [_img(0, [(0, 0, 10, 10, .9, 0)], [(0, 0, 10, 10, 0, 1), (0, 0, 10, 16, 0, 0)])], "bbox", 1, [0.5], DEFAULT


def crowd_matched_twice():
    """two detections inside one crowd gt: both match it, both are ignored; the plain gt elsewhere stays unmatched"""
    return [_img(0, [(0, 0, 10, 10, .9, 0), (10, 10, 20, 20, .8, 0)], [(0, 0, 20, 20, 0, 1), (50, 50, 60, 60, 0, 0)])], "bbox", 1, [0.5], DEFAULT


def unmatched_outside_range():
    """an unmatched detection of area 100: ignored in 'medium' and 'large', a false positive in 'all' and 'small'"""
    return [_img(0, [(0, 0, 10, 10, .9, 0)], [(50, 50, 90, 90, 0, 0)])], "bbox", 1, [0.5], DEFAULT


def area_edges():
    """gt areas of exactly 32^2 and 96^2: each counts in both ranges it borders"""
    return [_img(0, [(0, 0, 32, 32, .9, 0), (0, 0, 96, 96, .8, 1)], [(0, 0, 32, 32, 0, 0), (0, 0, 96, 96, 1, 0)])], "bbox", 2, [0.5], DEFAULT


def mask_half():
    """a mask IoU of exactly 2 / 4 matches at 0.5 (7 x 9 image: one word with a tail)"""
    px = _pixels(7, 9, [(1, 1), (1, 2)], [(1, 1), (1, 2), (1, 3), (1, 4)])
    return [_img(0, [(1, 1, 3, 2, .9, 0)], [(1, 1, 5, 2, 0, 0)], masks=px[:1], gt_masks=px[1:], height=7, width=9)], "segm", 1, [0.5], DEFAULT


def iou_one_at_one():
    """identical boxes: IoU exactly 1 matches at t = 1.0 (the threshold is min(t, 1 - 1e-10))"""
    return [_img(0, [(2, 3, 40, 50, .9, 0)], [(2, 3, 40, 50, 0, 0)])], "bbox", 1, [1.0], DEFAULT


def recall_past_the_end():
    """two gts, one true positive: recall 1 / 2; the recall thresholds above 0.5 find no position and read 0"""
    return [_img(0, [(0, 0, 10, 10, .9, 0)], [(0, 0, 10, 10, 0, 0), (50, 50, 60, 60, 0, 0)])], "bbox", 1, [0.5], DEFAULT


def no_counted_gt():
    """class 0 has only a crowd gt, class 1 none at all (and a detection): npig = 0, everything -1; class 2 is ordinary"""
    return [_img(0, [(0, 0, 10, 10, .9, 0), (0, 0, 10, 10, .9, 1), (30, 30, 50, 50, .7, 2)],
                 [(0, 0, 10, 10, 0, 1), (30, 30, 50, 50, 2, 0)])], "bbox", 3, [0.5], DEFAULT


def max_dets_per_cell():
    """two classes, each with its gt matched by its best detection and a worse one first in the image: at maxDets[0] = 1 each CELL keeps one"""
    return [_img(0, [(0, 0, 10, 10, .9, 0), (0, 0, 10, 11, .5, 0), (50, 50, 70, 70, .8, 1), (50, 50, 70, 71, .4, 1)],
                 [(0, 0, 10, 10, 0, 0), (50, 50, 70, 70, 1, 0)])], "bbox", 2, [0.5], (1, 2, 3)


HAND = dict(equal_iou_later_wins=equal_iou_later_wins, non_ignored_before_ignored=non_ignored_before_ignored, crowd_matched_twice=crowd_matched_twice,
            unmatched_outside_range=unmatched_outside_range, area_edges=area_edges, mask_half=mask_half, iou_one_at_one=iou_one_at_one,
            recall_past_the_end=recall_past_the_end, no_counted_gt=no_counted_gt, max_dets_per_cell=max_dets_per_cell)
