"""Input sets of the box-operator tests and the conditions they must meet, from the float64 reference (box_ref) alone.  Plain helper module.  The GPU
tests compare index lists exactly, so no decision of the reference may hang on less than the float32 kernels resolve:
  * NMS sets: no pair has its IoU within NMS_GAP of a threshold; no equal scores;
  * assignment sets (ASSIGN_GAP): no per-prior maximum within the gap of a threshold; no two overlaps compete for a per-prior arg-max within the gap
    unless both are 0; no two compete for a per-gt maximum within the gap unless the priors are exact duplicates; no per-gt maximum within the gap of a
    min_pos_iou.
Boxes are 8-64 px on a 256 x 256 canvas, rounded to float32.  The seeds are the first that pass (tests/test_box_host.py asserts the conditions)."""
import functools

import numpy as np

import box_ref as R

CANVAS, SMIN, SMAX = 256.0, 8.0, 64.0
NMS_GAP, ASSIGN_GAP = 1e-3, 1e-4
NMS_THRS = {False: (0.3, 0.5, 0.7, 0.8), True: (0.1, 0.5, 0.7, 0.8)}      # by `rotated`
ASSIGN_THRS = (0.1, 0.3, 0.5, 0.7)
NMS_SIZES = {False: (1, 2, 63, 64, 65, 128, 129), True: (1, 2, 63, 64, 65)}
ASSIGN_SIZES = ((1, 1), (3, 65), (65, 64), (65, 1000))
# the assigner configurations: the four of oriented_rcnn.py:78-108 / mask_rcnn.py:72-99, one without gt_max_assign_all, one with a neg_iou_thr pair
ASSIGN_CFGS = {
    "rpn": dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, gt_max_assign_all=True),
    "rcnn_off": dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, gt_max_assign_all=True),
    "rcnn_on": dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=True, gt_max_assign_all=True),
    "first_only": dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, gt_max_assign_all=False),
    "neg_pair": dict(pos_iou_thr=0.7, neg_iou_thr=(0.1, 0.3), min_pos_iou=0.3, match_low_quality=True, gt_max_assign_all=True),
}


def f32(a):
    return np.asarray(a, np.float32)


def rand_boxes(n, rng, rotated):
    c = rng.uniform(SMAX / 2, CANVAS - SMAX / 2, (n, 2))
    wh = rng.uniform(SMIN, SMAX, (n, 2))
    if rotated:
        return f32(np.concatenate([c, wh, rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1))
    return f32(np.concatenate([c - wh / 2, c + wh / 2], 1))


def iou64(boxes1, boxes2, rotated):
    return R.box_iou_rotated(boxes1, boxes2) if rotated else R.bbox_overlaps(boxes1, boxes2)


def clear_of(values, thrs, gap):
    v = np.asarray(values, np.float64).reshape(-1, 1)
    return bool((np.abs(v - np.asarray(thrs, np.float64)[None]) > gap).all())


# ------------------------------------------------------------------------------------------------------------------- NMS
def nms_condition(boxes, scores, rotated):
    iou = iou64(boxes, boxes, rotated)
    return clear_of(iou[np.triu_indices(len(boxes), 1)], NMS_THRS[rotated], NMS_GAP) and len(np.unique(scores)) == len(scores)


def _nms_try(n, seed, rotated):
    rng = np.random.default_rng(seed)
    boxes = rand_boxes(n, rng, rotated)
    scores = f32(rng.permutation(n) / max(n, 1) + 0.01)
    groups = rng.integers(0, 3, n).astype(np.int64)
    return boxes, scores, groups


def first_seed(make, passes, tries=400):
    for seed in range(tries):
        if passes(make(seed)):
            return seed
    raise AssertionError("no seed in %d passes: spread the boxes out, do not shrink the gap" % tries)


# the first seeds that pass, found with first_seed (python tests/box_cases.py prints both tables); the sets below assert their condition again
NMS_SEEDS = {(False, 1): 0, (False, 2): 0, (False, 63): 2, (False, 64): 0, (False, 65): 1, (False, 128): 3, (False, 129): 48,
             (True, 1): 0, (True, 2): 0, (True, 63): 1, (True, 64): 0, (True, 65): 0}


@functools.lru_cache(maxsize=None)
def nms_set(n, rotated):
    """(boxes, scores, groups)"""
    boxes, scores, groups = _nms_try(n, NMS_SEEDS[(rotated, n)], rotated)
    assert nms_condition(boxes, scores, rotated), (n, rotated)
    return boxes, scores, groups


CHAIN_LEN, CHAIN_N, CHAIN_N_WIDE = 64, 2049, 4225      # 33 mask words per row; 67: the scan's lanes take a second stride over the column blocks


@functools.lru_cache(maxsize=None)
def chain_set(rotated, n=CHAIN_N):
    """n boxes of 10 x 10 in rows of 64 (and one of 1), unit-shifted along their own axis, the rows 100 px apart, the scores shuffled; rotated: the
    whole scene turned by 0.3 rad.  Overlaps within a row are (10 - d) / (10 + d), across rows 0: long suppression chains over many mask words."""
    i = np.arange(n)
    x, y = 5.0 + (i % CHAIN_LEN), 5.0 + 100.0 * (i // CHAIN_LEN)
    rng = np.random.default_rng(5)
    scores = f32(rng.permutation(n) / n + 0.01)
    if not rotated:
        return f32(np.stack([x - 5, y - 5, x + 5, y + 5], 1)), scores
    t = 0.3
    return f32(np.stack([x * np.cos(t) - y * np.sin(t), x * np.sin(t) + y * np.cos(t), np.full(n, 10.0), np.full(n, 10.0), np.full(n, t)], 1)), scores


def chain_margins(rotated):
    """the distance of the chain set's overlap values (10 - d) / (10 + d), d = 0 .. 10, from each threshold"""
    v = (10.0 - np.arange(11)) / (10.0 + np.arange(11))
    return {t: float(np.abs(v - t).min()) for t in NMS_THRS[rotated]}


# ------------------------------------------------------------------------------------------------------------------- assignment
def hbox_to_rbox(h, angle):
    h = np.asarray(h, np.float64)
    return (np.stack([(h[:, 0] + h[:, 2]) / 2, (h[:, 1] + h[:, 3]) / 2, h[:, 2] - h[:, 0], h[:, 3] - h[:, 1], angle], 1))


def _assign_try(K, N, seed, kind):
    """gts of the calculator's kind; priors: the first min(K, N) are jittered gts (so that every regime from background to positive occurs), the rest random"""
    rng = np.random.default_rng(1000 + seed)
    grot, prot = kind != "box", kind == "rotated"
    gts = rand_boxes(K, rng, grot)
    priors = rand_boxes(N, rng, prot)
    m = min(K, N)
    base = gts[:m].astype(np.float64)
    if grot and not prot:
        base = R.rbox2hbox(base)
    jit = rng.uniform(-1.0, 1.0, (m, base.shape[1])) * np.linspace(0.5, 12.0, m)[:, None]
    if prot:
        jit[:, 4] *= 0.02
    priors[:m] = f32(base + jit)
    if not prot:
        priors[:, 2:] = np.maximum(priors[:, 2:], priors[:, :2] + 1)
    else:
        priors[:, 2:4] = np.maximum(priors[:, 2:4], 1)
    labels = rng.integers(0, 15, K).astype(np.int64)
    return gts, f32(priors), labels


def assign_condition(ov):
    """ov: the float64 (K, N) matrix"""
    K, N = ov.shape
    mx = ov.max(0)
    if not clear_of(mx, ASSIGN_THRS, ASSIGN_GAP):
        return False
    if K > 1:
        top = np.sort(ov, 0)[-2:]
        if not bool(((top[1] - top[0] > ASSIGN_GAP) | (top[1] == 0)).all()):
            return False
    gmx = ov.max(1)
    if not clear_of(gmx, ASSIGN_THRS + (0.0,), ASSIGN_GAP):
        return False
    if N > 1:
        top = np.sort(ov, 1)[:, -2:]
        if not bool((top[:, 1] - top[:, 0] > ASSIGN_GAP).all()):
            return False
    return True


ASSIGN_SEEDS = {("box", 1, 1): 0, ("box", 3, 65): 0, ("box", 65, 64): 0, ("box", 65, 1000): 1,
                ("rbox2hbox", 1, 1): 0, ("rbox2hbox", 3, 65): 0, ("rbox2hbox", 65, 64): 0, ("rbox2hbox", 65, 1000): 6,
                ("rotated", 1, 1): 0, ("rotated", 3, 65): 0, ("rotated", 65, 64): 0, ("rotated", 65, 1000): 30}


@functools.lru_cache(maxsize=None)
def assign_set(K, N, kind):
    """(gts, priors, labels, ov64)"""
    gts, priors, labels = _assign_try(K, N, ASSIGN_SEEDS[(kind, K, N)], kind)
    ov = R.overlaps(gts, priors, kind)
    assert assign_condition(ov), (K, N, kind)
    return gts, priors, labels, ov


# ---- more gts than one LDS tile of the assignment kernels (256)
BIG_K, BIG_N, TILE = 300, 640, 256


def _big_try(seed, kind):
    """300 gts on a sparse 20 x 15 grid (60 px apart, boxes of 16-40 px: gts of different cells never meet), gt 256 an exact duplicate of gt 255 -- the
    pair straddles the tile boundary.  Priors: one jittered copy per gt that is a clear positive (overlap > 0.7), one shifted copy per gt between 0.3
    and 0.5 for every second gt, which only the low-quality rule can match, then background.  Prior 255 is an exact copy of the duplicated gt."""
    rng = np.random.default_rng(7000 + seed)
    grot, prot = kind != "box", kind == "rotated"
    cell = np.arange(BIG_K)
    c = np.stack([40.0 + 60.0 * (cell % 20), 40.0 + 60.0 * (cell // 20)], 1) + rng.uniform(-4, 4, (BIG_K, 2))
    wh = rng.uniform(16, 40, (BIG_K, 2))
    ang = rng.uniform(-np.pi / 2, np.pi / 2, (BIG_K, 1))
    gr = np.concatenate([c, wh, ang], 1)
    gr[TILE] = gr[TILE - 1]
    gts = f32(gr if grot else np.concatenate([gr[:, :2] - gr[:, 2:4] / 2, gr[:, :2] + gr[:, 2:4] / 2], 1))
    base = gts.astype(np.float64)
    if grot and not prot:
        base = R.rbox2hbox(base)

    def moved(b, d):      # centres moved by d (K, 2)
        out = b.copy()
        out[:, :2] += d
        if not prot:
            out[:, 2:4] += d
        return out
    size = (base[:, 2:4] if prot else base[:, 2:4] - base[:, :2])
    near = moved(base, rng.uniform(-0.03, 0.03, (BIG_K, 2)) * size)
    near[TILE - 1] = base[TILE - 1]
    low = moved(base, np.stack([0.42 * size[:, 0], np.zeros(BIG_K)], 1) if not prot else
                np.stack([0.42 * size[:, 0] * np.cos(base[:, 4]), 0.42 * size[:, 0] * np.sin(base[:, 4])], 1))[::2]
    # every second gt loses its positive: its best prior is the shifted copy
    keep_near = np.ones(BIG_K, bool)
    keep_near[::2] = False
    keep_near[[TILE - 1, TILE]] = True
    far = rand_boxes(BIG_N - BIG_K - len(low), rng, prot).astype(np.float64)
    far[:, :2] += [1300.0, 0.0]
    if not prot:
        far[:, 2:4] += [1300.0, 0.0]
    near[~keep_near, :2] += 5000.0
    if not prot:
        near[~keep_near, 2:4] += 5000.0
    priors = f32(np.concatenate([near, low, far]))
    labels = rng.integers(0, 15, BIG_K).astype(np.int64)
    return gts, priors, labels


def big_condition(ov):
    """assign_condition, with the one exemption its docstring names -- here for the exact duplicate gts TILE - 1 and TILE, whose rows are equal"""
    assert np.array_equal(ov[TILE - 1], ov[TILE])
    return assign_condition(np.delete(ov, TILE, 0))


BIG_SEEDS = {"box": 0, "rbox2hbox": 0, "rotated": 0}


@functools.lru_cache(maxsize=None)
def big_set(kind):
    """(gts, priors, labels, ov64) with K = 300 > 256"""
    gts, priors, labels = _big_try(BIG_SEEDS[kind], kind)
    ov = R.overlaps(gts, priors, kind)
    assert big_condition(ov), kind
    return gts, priors, labels, ov


if __name__ == "__main__":
    print({kind: first_seed(lambda s: _big_try(s, kind), lambda t: big_condition(R.overlaps(t[0], t[1], kind))) for kind in R.KINDS})
    print({(rot, n): first_seed(lambda s: _nms_try(n, s, rot), lambda t: nms_condition(t[0], t[1], rot)) for rot in (False, True) for n in NMS_SIZES[rot]})
    print({(kind, K, N): first_seed(lambda s: _assign_try(K, N, s, kind), lambda t: assign_condition(R.overlaps(t[0], t[1], kind)))
           for kind in R.KINDS for K, N in ASSIGN_SIZES})
