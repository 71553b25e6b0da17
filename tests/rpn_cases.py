"""Input sets of the oriented-RPN tests and the conditions they must meet, from the float64 reference (rpn_ref, box_ref) alone.  Plain helper module.
The GPU tests compare index lists exactly, so no decision of the reference may hang on less than the float32 kernels resolve:
  * no non-extreme corner of a gt box lies within CUT_GAP of the coder's 0.1 cut;
  * no decoded proposal has |w - h| < SHAPE_GAP max(w, h) or theta within SHAPE_GAP of +-pi/2 (the edge choice and the fold);
  * no two scores that straddle a level's nms_pre cut, or are adjacent in the NMS order, are closer than SCORE_GAP;
  * the assignment (inside anchors against the gts, RBbox2HBboxOverlaps2D) meets box_cases.assign_condition, and no pair of proposals of one level
    has its overlap within box_cases.NMS_GAP of the NMS threshold;
  * the square case has a positive through pos_iou_thr and one only through the low-quality match; one image has more positives than the sampler's cap.
The configuration is oriented_rcnn.py:20-40, 77-99 shrunk to num=16, nms_pre=100, max_per_img=50.  The seeds are the first that pass
(tests/test_rpn_host.py asserts the conditions)."""
import functools

import numpy as np

import box_cases as BC
import box_ref as BR
import rpn_ref as R

CUT_GAP, SHAPE_GAP, SCORE_GAP = 1e-3, 1e-3, 1e-6
STRIDES, SCALES, RATIOS, A = (4, 8, 16, 32, 64), (8,), (0.5, 1.0, 2.0), 3
MEANS, STDS = (0.0,) * 6, (1.0, 1.0, 1.0, 1.0, 0.5, 0.5)
BETA = 0.1111111111111111
ASSIGNER = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1)
NUM, POS_FRACTION = 16, 0.5
PROPOSAL = dict(nms_pre=100, max_per_img=50, nms=dict(type="nms", iou_threshold=0.8), min_bbox_size=0)
MIN_SIZE = 24      # the second proposal run: a min_bbox_size that removes boxes
BATCH, NUM_GT = 2, 6
# name -> (img_shape, pad_shape, gts per image)
SHAPES = {"sq128": ((128, 128), (128, 128), (NUM_GT, NUM_GT)), "pad160": ((96, 160), (128, 160), (NUM_GT, 0))}


def sizes_of(pad_shape):
    return [(-(-pad_shape[0] // s), -(-pad_shape[1] // s)) for s in STRIDES]


@functools.lru_cache(maxsize=None)
def anchors(name, dtype=np.float64):
    """(flat priors (n, 4), inside flags (n) bool, sizes)"""
    img, pad, _ = SHAPES[name]
    sizes = sizes_of(pad)
    pr, fl = [], []
    for (H, W), s in zip(sizes, STRIDES):
        p = R.grid_priors(R.base_anchors(s, SCALES, RATIOS), H, W, (s, s), dtype)
        pr.append(p)
        fl.append(R.inside_flags(p, A, H, W, (s, s), pad, img, 0))
    return np.concatenate(pr), np.concatenate(fl), sizes


def _try(name, seed):
    """cls maps [(B, A, H, W)], reg maps [(B, 6 A, H, W)] float32, gts per image (K, 5) float32"""
    rng = np.random.default_rng(2200 + seed)
    img, _, counts = SHAPES[name]
    priors, inside, sizes = anchors(name)
    cls = [BC.f32(rng.normal(0.0, 1.5, (BATCH, A, H, W))) for H, W in sizes]
    reg = []
    for H, W in sizes:      # offsets and log sizes N(0, 0.3); the two midpoint offsets uniform inside the coder's clamp (raw * std 0.5 within +-0.475)
        r = rng.normal(0.0, 0.3, (BATCH, A, 6, H, W))
        r[:, :, 4:] = rng.uniform(-0.95, 0.95, (BATCH, A, 2, H, W))
        reg.append(BC.f32(r.reshape(BATCH, 6 * A, H, W)))
    cand = priors[inside]
    gts = []
    for k in counts:
        g = np.zeros((k, 5))
        for i in range(k):      # an anchor, resized and turned a little and moved by up to a pixel: positives through pos_iou_thr
            ax = int(rng.integers(2))
            shape = cand[:, 2 + ax] - cand[:, ax] < cand[:, 3 - ax] - cand[:, 1 - ax] if i % 2 else np.ones(len(cand), bool)
            p = cand[shape][rng.integers(int(shape.sum()))]
            wh = (p[2:] - p[:2]) * rng.uniform(0.92, 1.0, 2)
            c = np.array([(p[0] + p[2]) / 2, (p[1] + p[3]) / 2]) + rng.uniform(-1, 1, 2)
            if i % 2:           # the odd ones, their short side across the right or the lower border, hang over it by a quarter of that side: the
                c[ax] = img[1 - ax] - wh[ax] / 2 + rng.uniform(0.2, 0.3) * wh[ax]      # anchors that fit them are not inside the image, the best one
            g[i] = [c[0], c[1], wh[0], wh[1], rng.uniform(-0.08, 0.08)]                 # left is a low-quality match
        gts.append(BC.f32(g))
    return cls, reg, gts


def assign64(name, gts):
    """the reference's assignment of one image on the anchors inside it -> (gt_inds, max overlaps, the (K, N) matrix)"""
    priors, inside, _ = anchors(name)
    ov = BR.overlaps(np.asarray(gts, np.float64), priors[inside], "rbox2hbox") if len(gts) else np.zeros((0, int(inside.sum())))
    cfg = {k: v for k, v in ASSIGNER.items() if k != "ignore_iof_thr"}
    gt_inds, mx, _ = BR.assign_wrt_overlaps(ov, np.zeros(len(gts), np.int64), **cfg)
    return gt_inds, mx, ov


def corner_condition(gts):
    X, Y = R.corners(gts)
    dy, dx = np.abs(Y - Y.min(1, keepdims=True)), np.abs(X - X.max(1, keepdims=True))
    return bool((np.abs(dy - 0.1) > CUT_GAP).all() and (np.abs(dx - 0.1) > CUT_GAP).all())


def proposal_condition(name, cls, reg):
    priors, _, sizes = anchors(name)
    for b in range(BATCH):
        cb, rb = [m[b] for m in cls], [m[b] for m in reg]
        for m in cb:      # the nms_pre cut
            z = np.sort(1.0 / (1.0 + np.exp(-np.transpose(m, (1, 2, 0)).reshape(-1).astype(np.float64))))[::-1]
            k = PROPOSAL["nms_pre"]
            if k < len(z) and not z[k - 1] - z[k] > SCORE_GAP:
                return False
        keep = R.topk_per_level(cb, PROPOSAL["nms_pre"])
        sc, rbx, hb, ids = R.decode_kept(cb, rb, priors, sizes, A, keep, MEANS, STDS)
        s = np.sort(sc)
        if len(s) > 1 and not (np.diff(s) > SCORE_GAP).all():
            return False
        w, h, t = rbx[:, 2], rbx[:, 3], rbx[:, 4]
        if (np.abs(w - h) < SHAPE_GAP * np.maximum(w, h)).any() or (np.abs(np.abs(t) - np.pi / 2) < SHAPE_GAP).any():
            return False
        if (np.abs(w - MIN_SIZE) < SHAPE_GAP).any() or (np.abs(h - MIN_SIZE) < SHAPE_GAP).any():
            return False
        for l in range(len(sizes)):
            hl = hb[ids == l]
            iou = BR.bbox_overlaps(hl, hl)[np.triu_indices(len(hl), 1)]
            if not BC.clear_of(iou, (PROPOSAL["nms"]["iou_threshold"],), BC.NMS_GAP):
                return False
    return True


def condition(name, case):
    cls, reg, gts = case
    both = more = False
    for g in gts:
        if len(g) == 0:
            continue
        if not corner_condition(g):
            return False
        gt_inds, mx, ov = assign64(name, g)
        if not BC.assign_condition(ov):
            return False
        pos = gt_inds > 0
        both = both or bool((pos & (mx >= ASSIGNER["pos_iou_thr"])).any() and (pos & (mx < ASSIGNER["pos_iou_thr"])).any())
        more = more or int(pos.sum()) > int(NUM * POS_FRACTION)
    if name == "sq128" and not (both and more):
        return False
    return proposal_condition(name, cls, reg)


SEEDS = {"sq128": 45, "pad160": 136}


@functools.lru_cache(maxsize=None)
def case(name):
    """(cls maps, reg maps, gts per image)"""
    c = _try(name, SEEDS[name])
    assert condition(name, c), name
    return c


def metas(name):
    img, pad, _ = SHAPES[name]
    return [dict(img_shape=img, pad_shape=pad) for _ in range(BATCH)]


if __name__ == "__main__":
    print({n: BC.first_seed(lambda s: _try(n, s), lambda c: condition(n, c)) for n in SHAPES})
