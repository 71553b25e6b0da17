"""Input sets of the DOTA-metric tests and the conditions they must meet, from the float64 reference (box_ref / det_eval_ref) alone.  Plain helper
module.  The GPU tests compare flags and indices exactly, so no decision of the reference may hang on less than the float32 kernels resolve.  A whole
seed is rejected (box_cases.first_seed) unless, for every image and class,
  * no IoU of a detection with a gt of its class lies within GAP of a threshold in THRS;
  * the two largest IoUs of a detection are at least GAP apart (both 0 is the one exemption: disjoint boxes give an exact 0 in either precision);
  * the scores of a class are pairwise distinct;
  * every box side is at least MIN_SIDE px.
The constructed cases (ties, the exact family) are not random and carry their own argument.  Scenes are sparse: the gts sit in cells 120 px apart
(boxes of 8-64 px, so different cells never meet), every seventh gt shares its cell with a shifted copy of its neighbour -- overlapping gts, so that the
arg-max decides -- and the detections are jittered copies of gts (none to three per gt) plus background boxes with random labels.  Boxes are rounded to
float32.  The seeds are the first that pass (tests/test_det_eval_host.py asserts the conditions)."""
import functools

import numpy as np

import box_cases as BC
import box_ref as BR
import det_eval_ref as R

GAP, MIN_SIDE, CELL = 1e-3, 4.0, 120.0
THRS = (0.3, 0.5, 0.75)          # every threshold a test uses


def _rbox(rng, cell):
    c = np.array([cell % 12, cell // 12]) * CELL + 60.0 + rng.uniform(-10, 10, 2)
    return np.concatenate([c, rng.uniform(8.0, 64.0, 2), rng.uniform(-np.pi / 2, np.pi / 2, 1)])


def _try(seed, gts_per_image, K, D=None, ignore_every=4, no_det_images=()):
    """-> (det_results, annotations): det_results[i][k] (m, 6) float64 holding float32 values, annotations[i] = bboxes / labels / bboxes_ignore /
    labels_ignore.  Every ignore_every-th gt is ignored (0: none); with D the detections are cut or filled up to exactly D."""
    rng = np.random.default_rng(24000 + seed)
    anns, dets = [], []          # dets: (image, label, box)
    for i, n in enumerate(gts_per_image):
        boxes = np.zeros((n, 5))
        for j in range(n):
            boxes[j] = _rbox(rng, j)
            if j % 7 == 6:           # an overlapping pair: a shifted copy of the neighbour in the neighbour's cell
                boxes[j] = boxes[j - 1] + np.array([0.45 * boxes[j - 1, 2] * np.cos(boxes[j - 1, 4]), 0.45 * boxes[j - 1, 2] * np.sin(boxes[j - 1, 4]), 0, 0, 0])
        boxes = BC.f32(boxes).astype(np.float64)
        labels = rng.integers(0, K, n).astype(np.int64)
        ign = (np.arange(n) % ignore_every == ignore_every - 1) if ignore_every else np.zeros(n, bool)
        anns.append(dict(bboxes=boxes[~ign], labels=labels[~ign], bboxes_ignore=boxes[ign], labels_ignore=labels[ign]))
        if i in no_det_images:
            continue
        for j in range(n):
            for _ in range(int(rng.choice([0, 1, 1, 2, 3]))):
                jit = rng.uniform(-1, 1, 5) * np.array([0.25 * boxes[j, 2], 0.25 * boxes[j, 3], 0.2 * boxes[j, 2], 0.2 * boxes[j, 3], 0.15])
                dets.append((i, int(labels[j]), boxes[j] + jit))
        for _ in range(max(2, n // 4)):
            dets.append((i, int(rng.integers(0, K)), _rbox(rng, int(rng.integers(0, max(n, 4))))))
    if D is not None:
        live = [i for i in range(len(gts_per_image)) if i not in no_det_images]
        while len(dets) < D:
            i = live[len(dets) % len(live)]
            dets.append((i, int(rng.integers(0, K)), _rbox(rng, int(rng.integers(0, max(gts_per_image[i], 4))))))
        dets = sorted(dets[:D], key=lambda d: d[0])
    scores = (rng.permutation(len(dets)) + 1.0) / (len(dets) + 1.0)
    res = [[[] for _ in range(K)] for _ in gts_per_image]
    for (i, k, b), s in zip(dets, scores):
        b = b.copy()
        b[2:4] = np.maximum(b[2:4], MIN_SIDE)
        res[i][k].append(np.concatenate([b, [s]]))
    res = [[BC.f32(np.asarray(r).reshape(-1, 6)).astype(np.float64) for r in img] for img in res]
    return res, anns


def condition(case, thrs=THRS):
    det_results, annotations = case
    for res, ann in zip(det_results, annotations):
        for k, d in enumerate(res):
            if len(np.unique(d[:, 5])) != len(d) or (len(d) and d[:, 2:4].min() < MIN_SIDE):
                return False
            g = np.vstack([ann["bboxes"][ann["labels"] == k], ann["bboxes_ignore"][ann["labels_ignore"] == k]])
            if len(g) and g[:, 2:4].min() < MIN_SIDE:
                return False
            if not len(d) or not len(g):
                continue
            iou = BR.box_iou_rotated(d[:, :5], g)
            if not BC.clear_of(iou, thrs, GAP):
                return False
            if len(g) > 1:
                top = np.sort(iou, 1)[:, -2:]
                if not bool(((top[:, 1] - top[:, 0] >= GAP) | (top[:, 1] == 0)).all()):
                    return False
    # distinct within a class over the whole set: the global sort of eval_rbbox_map
    for k in range(len(det_results[0])):
        s = np.concatenate([res[k][:, 5] for res in det_results])
        if len(np.unique(s)) != len(s):
            return False
    return True


# name -> (gts per image, classes, D or None, images without detections)
SPECS = {
    "fixture": ((5, 0, 3, 8, 1, 12), 4, None, ()),
    "gts_0_1": ((0, 1, 3), 3, None, ()),
    "gts_63_64_65": ((63, 64, 65), 5, None, ()),
    "gts_130": ((130, 2), 5, None, (1,)),
    "dets_1": ((3,), 2, 1, ()),
    "dets_255": ((40, 30), 15, 255, ()),
    "dets_256": ((40, 30), 15, 256, ()),
    "dets_257": ((40, 30, 5), 15, 257, (2,)),
}
# the first seeds that pass (python tests/det_eval_cases.py prints the table); case() asserts the condition again
SEEDS = {"fixture": 0, "gts_0_1": 0, "gts_63_64_65": 1, "gts_130": 1, "dets_1": 0, "dets_255": 0, "dets_256": 0, "dets_257": 0}


def ignore_rule(name):
    return 3 if name == "fixture" else 4


def make(name, seed):
    gts, K, D, nodet = SPECS[name]
    res, anns = _try(seed, gts, K, D, ignore_rule(name), nodet)
    if name == "fixture":          # image 2: nothing but ignored gts -- it counts as an image without gts, its detections are all false positives
        a = anns[2]
        anns[2] = dict(bboxes=a["bboxes"][:0], labels=a["labels"][:0], bboxes_ignore=np.vstack([a["bboxes"], a["bboxes_ignore"]]),
                       labels_ignore=np.concatenate([a["labels"], a["labels_ignore"]]))
    return res, anns


@functools.lru_cache(maxsize=None)
def case(name):
    """(det_results, annotations)"""
    c = make(name, SEEDS[name])
    assert condition(c), name
    return c


@functools.lru_cache(maxsize=None)
def expected(name, thrs):
    """det_eval_ref.table_results of a case, computed once and shared"""
    return R.table_results(*case(name), list(thrs))


# ------------------------------------------------------------------------------------------------------------------- constructed cases
def _ann(boxes, labels, ign_boxes=(), ign_labels=()):
    return dict(bboxes=np.asarray(boxes, np.float64).reshape(-1, 5), labels=np.asarray(labels, np.int64).reshape(-1),
                bboxes_ignore=np.asarray(ign_boxes, np.float64).reshape(-1, 5), labels_ignore=np.asarray(ign_labels, np.int64).reshape(-1))


G0 = [100.0, 100.0, 40.0, 20.0, 0.25]


def shifted(b, dx, score=None):
    out = [b[0] + dx * np.cos(b[4]), b[1] + dx * np.sin(b[4])] + list(b[2:5])
    return out if score is None else out + [score]


def ties_case():
    """one class, one image.  gt 0 takes three detections (IoU 0.9, 0.8, 0.7 along its axis; scores 0.5, 0.9, 0.9: the two 0.9s tie and the lower
    index, row 1, is the true positive); gt 1 takes two with distinct scores; the best match of row 5 is an ignored gt (neither tp nor fp at 0.5)."""
    g1, g2 = [300.0, 100.0, 30.0, 30.0, -0.4], [500.0, 100.0, 50.0, 16.0, 1.0]
    dets = [shifted(G0, 40 * (1 - 0.9) / (1 + 0.9), 0.5), shifted(G0, 40 * (1 - 0.8) / (1 + 0.8), 0.9), shifted(G0, 40 * (1 - 0.7) / (1 + 0.7), 0.9),
            shifted(g1, 3.0, 0.3), shifted(g1, 1.0, 0.6), shifted(g2, 2.0, 0.95), [700.0, 700.0, 20.0, 20.0, 0.0, 0.99]]
    return [[BC.f32(dets).astype(np.float64)]], [_ann([G0, g1], [0, 0], [g2], [0])]


def voc_case():
    """gts a and b overlap; detection 0 (score 0.9) sits on a; detection 1 (score 0.8) lies between them with IoU(a) > IoU(b) > 0.5: its arg-max a is
    covered, so it is a false positive although b is free and clears the threshold"""
    a, b = [100.0, 100.0, 40.0, 40.0, 0.0], [112.0, 100.0, 40.0, 40.0, 0.0]
    dets = [[100.0, 100.0, 40.0, 40.0, 0.0, 0.9], [105.0, 100.0, 40.0, 40.0, 0.0, 0.8]]
    return [[BC.f32(dets).astype(np.float64)]], [_ann([a, b], [0, 0])]


def exact_case():
    """dyadic boxes at theta = 0: the gt (8..24) x (8..24) inside the detection (8..40) x (8..24): intersection 256, union 512, IoU exactly 0.5 in
    float32 and float64 -- `>=` matches at iou_thr = 0.5.  The second pair has IoU exactly 0.25 (256 / 1024)."""
    gts = [[16.0, 16.0, 16.0, 16.0, 0.0], [216.0, 16.0, 16.0, 16.0, 0.0]]
    dets = [[24.0, 16.0, 32.0, 16.0, 0.0, 0.75], [240.0, 16.0, 64.0, 16.0, 0.0, 0.5]]
    return [[BC.f32(dets).astype(np.float64)]], [_ann(gts, [0, 0])]


def recall_quirk_flags(hits):
    """flags of one class with num_gts = 10: `hits` true positives first, then five false positives: the last recall is exactly hits / 10"""
    return np.array([R.TP] * hits + [R.FP] * 5, np.uint8)


if __name__ == "__main__":
    print({n: BC.first_seed(lambda s: make(n, s), condition) for n in SPECS})
