"""Seeded inputs of the mask-branch tests (tests/test_mask_host.py, tests/test_hip_mask.py, tests/golden/make_mask_branch.py) and their CPU run.

Sizes are chosen for the seams, not the workload: 64 x 64 images, batch 2, maps 16 / 8 / 4 / 2 (strides 4 .. 32), C = 8 (one case C = 5: no multiple of
a lane chunk), K = 3 classes, S = 8 sample slots per image, RoIAlign 14 -> mask 28.  finest_scale is 16, not 56, so that boxes inside a 64-pixel image
reach every level.  The ground truths are irregular blobs.  The positives of image 0: the gts' own integer boxes (add_gt_as_proposals), a box reaching
outside on the left / top, one on the right / bottom, a box larger than the image (level 3; adaptive grid 3 on the bitmaps), a thin box of ratio > 8
and a zero-width box.  Image 1: its gts' boxes and two jittered ones.  'one_empty': image 1 has no positive; 'none': no positive at all.

Thresholds decide bits, so every case's seed is searched (search()) until no float64 target average and no pasted value lies within MARGIN of its
threshold; the seeds found are pinned in SHAPES and case() asserts nothing.  make_mask_branch.py asserts the margins when it writes the fixture."""
import numpy as np
import torch
import torch.nn.functional as F

import mask_ref as MR

IMG, BATCH, STRIDES, K, S, OUT, M, FINEST, CONV = 64, 2, (4, 8, 16, 32), 3, 8, 14, 28, 16.0, 8
NUM_CONVS, LOSS_WEIGHT, THR, MARGIN = 4, 1.0, 0.5, 1e-4
PASTE_HW, PASTE_SCALE = (37, 53), (1.25, 0.8)      # ori_shape (h, w); scale_factor (w, h)
SHAPES = {
    "base": dict(C=8, seed=102, empty=()),
    "odd": dict(C=5, seed=277, empty=()),
    "one_empty": dict(C=8, seed=321, empty=(1,)),
    "none": dict(C=8, seed=401, empty=(0, 1)),
}
NUM_GTS = (2, 3)


def blob(rng):
    """an irregular 64 x 64 bitmap: a union of three ellipses with a ragged rim -> (bitmap uint8, its integer box x1, y1, x2, y2)"""
    yy, xx = np.mgrid[0:IMG, 0:IMG].astype(np.float64)
    cy, cx = rng.uniform(18, 46, 2)
    m = np.zeros((IMG, IMG), bool)
    for _ in range(3):
        oy, ox = rng.uniform(-7, 7, 2)
        ry, rx = rng.uniform(4, 11, 2)
        m |= ((yy - cy - oy) / ry) ** 2 + ((xx - cx - ox) / rx) ** 2 <= 1.0 + 0.35 * rng.standard_normal((IMG, IMG))
    m &= ((yy - cy) ** 2 + (xx - cx) ** 2) <= 20.0 ** 2
    ys, xs = np.nonzero(m)
    return m.astype(np.uint8), np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32)


def build(name, seed):
    cfg = SHAPES[name]
    rng = np.random.default_rng(seed)
    Cc = cfg["C"]
    feats = [rng.standard_normal((BATCH, Cc, IMG // s, IMG // s)).astype(np.float32) for s in STRIDES]
    bitmaps, gt_boxes, gt_labels, gt_start = [], [], [], [0]
    for b in range(BATCH):
        for _ in range(NUM_GTS[b]):
            m, box = blob(rng)
            bitmaps.append(m)
            gt_boxes.append(box)
            gt_labels.append(rng.integers(0, K))
        gt_start.append(len(bitmaps))
    bitmaps, gt_boxes, gt_labels = np.stack(bitmaps), np.stack(gt_boxes), np.array(gt_labels, np.int64)
    special = np.array([[-12.3, -9.2, 34.5, 30.7], [25.2, 20.1, 90.6, 99.3], [-40.0, -35.0, 100.0, 95.0], [5.2, 30.1, 53.6, 35.9], [22.5, 10.0, 22.5, 40.0]], np.float32)
    pos = []
    for b in range(BATCH):
        own = gt_boxes[gt_start[b]:gt_start[b + 1]]
        if b == 0:
            boxes, gt = np.concatenate([own, special]), np.concatenate([np.arange(len(own)), rng.integers(0, len(own), len(special))])
        else:
            jit = own[:2] + rng.uniform(-3.5, 3.5, (2, 4)).astype(np.float32)
            boxes, gt = np.concatenate([own, jit]), np.concatenate([np.arange(len(own)), np.arange(2)])
        if b in cfg["empty"]:
            boxes, gt = boxes[:0], gt[:0]
        pos.append(dict(boxes=boxes.astype(np.float32), gt=gt.astype(np.int64), labels=gt_labels[gt_start[b] + gt.astype(np.int64)]))
    # the fixed-slot form: the positives first; the padding slots hold plausible boxes and a row of -1
    boxes = rng.uniform(0, IMG / 2, (BATCH, S, 4)).astype(np.float32)
    boxes[:, :, 2:] += boxes[:, :, :2] + 4
    sample_gt, labels, n_pos = np.full((BATCH, S), -1, np.int64), np.zeros((BATCH, S), np.int64), np.zeros(BATCH, np.int64)
    for b, p in enumerate(pos):
        n = len(p["boxes"])
        assert n <= S
        boxes[b, :n], sample_gt[b, :n], labels[b, :n], n_pos[b] = p["boxes"], p["gt"] + gt_start[b], p["labels"], n
    rois = np.concatenate([np.repeat(np.arange(BATCH, dtype=np.float32), S)[:, None], boxes.reshape(-1, 4)], 1)
    w = {}
    for i in range(NUM_CONVS):
        cin = Cc if i == 0 else CONV
        w["convs.%d.conv.weight" % i] = (rng.standard_normal((CONV, cin, 3, 3)) * (1.4 / np.sqrt(9 * cin))).astype(np.float32)
        w["convs.%d.conv.bias" % i] = (rng.standard_normal(CONV) * 0.1).astype(np.float32)
    w["upsample.weight"] = (rng.standard_normal((CONV, CONV, 2, 2)) * (1.4 / np.sqrt(CONV))).astype(np.float32)
    w["upsample.bias"] = (rng.standard_normal(CONV) * 0.1).astype(np.float32)
    logits_w = dict(weight=(rng.standard_normal((K, CONV, 1, 1)) * (2.0 / np.sqrt(CONV))).astype(np.float32), bias=(rng.standard_normal(K) * 0.1).astype(np.float32))
    # the paste: 6 instances on the 37 x 53 image, in the scaled frame (boxes / scale_factor is the image frame)
    n_inst = 6
    coarse = rng.standard_normal((n_inst, K, 7, 7))
    pl = F.interpolate(torch.from_numpy(coarse), size=(M, M), mode="bilinear", align_corners=False).numpy() * 3.0 + 0.3 * rng.standard_normal((n_inst, K, M, M))
    sw, sh = PASTE_SCALE
    pb = np.array([[4.3, 3.1, 30.8, 25.6], [-5.5, 10.2, 18.4, 45.0], [35.7, 2.2, 70.9, 20.1], [10.0, 8.0, 10.0, 30.0], [20.3, 12.4, 22.0, 14.1], [0.0, 0.0, 53.0 * sw, 37.0 * sh]],
                  np.float32)
    return dict(name=name, C=Cc, feats=feats, bitmaps=bitmaps, gt_boxes=gt_boxes, gt_labels=gt_labels, gt_start=gt_start, pos=pos, rois=rois.astype(np.float32),
                boxes=boxes.reshape(-1, 4), sample_gt=sample_gt, labels=labels.reshape(-1), n_pos=n_pos, weights=w, conv_logits=logits_w,
                paste=dict(logits=pl.astype(np.float32), boxes=pb, labels=rng.integers(0, K, n_inst).astype(np.int64)))


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = build(name, SHAPES[name]["seed"])
    return _CASES[name]


def in_use(c):
    return (np.arange(S)[None, :] < c["n_pos"][:, None]).reshape(-1)


def paste_frames(c):
    """(rescale, boxes in the output frame, img_h, img_w): rescale divides the boxes by scale_factor and pastes at ori_shape; without it the
    boxes stay and the image is ori_shape * scale_factor, rounded"""
    sw, sh = PASTE_SCALE
    h, w = PASTE_HW
    b = c["paste"]["boxes"]
    return [(True, (b / np.array([sw, sh, sw, sh], np.float32)).astype(np.float32), h, w), (False, b, int(np.round(h * sh)), int(np.round(w * sw)))]


def targets(c, ft=np.float64):
    """the positives' targets in slot order -> (avg, targets) of the fixed slots (zeros on padding)"""
    use = in_use(c)
    avg, tg = np.zeros((BATCH * S, M, M), ft), np.zeros((BATCH * S, M, M), np.uint8)
    if use.any():
        a, t = MR.mask_targets(c["boxes"][use], c["sample_gt"].reshape(-1)[use], c["bitmaps"], M, ft=ft)
        avg[use], tg[use] = a, t
    return avg, tg


def margins(c):
    """(the smallest float64 distance of a target average from 0.5, of a pasted value from THR)"""
    use = in_use(c)
    avg, _ = targets(c)
    m_t = float(np.abs(avg[use] - 0.5).min()) if use.any() else 1.0
    m_p = 1.0
    for _, boxes, h, w in paste_frames(c):
        v, _ = MR.paste(c["paste"]["logits"], c["paste"]["labels"], boxes, h, w, THR)
        m_p = min(m_p, float(np.nanmin(np.abs(v - THR))))
    return m_t, m_p


def level_margin(c):
    """the distance of log2(scale / finest + 1e-6) from an integer over the RoIs in use with a positive scale: float32 and float64 agree on floor()"""
    r = c["rois"][in_use(c)].astype(np.float64)
    sc = np.sqrt(np.maximum((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]), 0))
    v = np.log2(sc[sc > 0] / FINEST + 1e-6)
    return float(np.abs(v - np.round(v)).min()) if v.size else 1.0


def search(name, tries=200):
    """the first seed from the case's base (a multiple of 100) whose margins hold"""
    base = SHAPES[name]["seed"] // 100 * 100
    for seed in range(base, base + tries):
        c = build(name, seed)
        if min(margins(c)) > MARGIN and level_margin(c) > 1e-3:
            return seed
    raise RuntimeError("no seed for %s" % name)


# ------------------------------------------------------------------------------------------------------------------- the CPU run
class _Align(torch.autograd.Function):
    """mask_ref's RoIAlign over all levels, forward and backward"""

    @staticmethod
    def forward(ctx, rois, use, ft, *feats):
        ctx.a = (rois, use, ft, [tuple(f.shape) for f in feats])
        out, _ = MR.roi_align([f.detach().numpy() for f in feats], rois, STRIDES, OUT, 0, True, FINEST, in_use=use, ft=ft)
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, dout):
        rois, use, ft, shapes = ctx.a
        g = MR.roi_align_bwd(dout.numpy(), shapes, rois, STRIDES, OUT, 0, True, FINEST, in_use=use, ft=ft)
        return (None, None, None) + tuple(torch.from_numpy(a) for a in g)


class _RoundGrad(torch.autograd.Function):
    """identity whose gradient is rounded to `dtype` and back: where the engine's 'bf16' mode keeps a gradient in bf16"""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def head_forward(x, W, L, round_to=None):
    """FCNMaskHead.forward + the external conv_logits, in torch.  round_to=torch.bfloat16: the engine's 'bf16' mode -- the operands of every layer
    (activations, weights) are rounded to bf16, sums are f32, and on the way back the gradient of every layer's output is rounded to bf16 before it
    meets the weight-gradient and data-gradient GEMMs"""
    q = (lambda t: t) if round_to is None else (lambda t: t.to(round_to).to(t.dtype))
    g = (lambda t: t) if round_to is None else (lambda t: _RoundGrad.apply(t, round_to))
    for i in range(NUM_CONVS):
        x = F.relu(g(F.conv2d(q(x), q(W["convs.%d.conv.weight" % i]), W["convs.%d.conv.bias" % i], padding=1)))
    x = F.relu(g(F.conv_transpose2d(q(x), q(W["upsample.weight"]), W["upsample.bias"], stride=2)))
    return g(F.conv2d(q(x), q(L["weight"]), L["bias"]))


def run(c, ft=np.float64, round_to=None):
    """the whole branch on the CPU in ft: levels, mask_feats, mask_preds, targets, loss_mask and the gradients of every map and parameter"""
    tt = torch.float64 if ft == np.float64 else torch.float32
    use = in_use(c)
    feats = [torch.from_numpy(f).to(tt).requires_grad_(True) for f in c["feats"]]
    W = {k: torch.from_numpy(v).to(tt).requires_grad_(True) for k, v in c["weights"].items()}
    L = {k: torch.from_numpy(v).to(tt).requires_grad_(True) for k, v in c["conv_logits"].items()}
    mask_feats = _Align.apply(c["rois"], use, ft, *feats)
    preds = head_forward(mask_feats, W, L, round_to)
    avg, tg = targets(c, ft)
    n_total = int(c["n_pos"].sum())
    out = dict(levels=MR.map_roi_levels(c["rois"], FINEST, len(STRIDES), ft), mask_feats=mask_feats.detach().numpy(), mask_preds=preds.detach().numpy(),
               target_avg=avg, targets=tg)
    channels = np.where(use, c["labels"], -1)
    loss, slot, d = MR.mask_loss(preds.detach().numpy(), tg, channels, n_total, LOSS_WEIGHT, ft)
    out.update(loss_mask=np.asarray(loss, ft), slot_loss=slot, dlogits=d)
    preds.backward(torch.from_numpy(d))
    zero = lambda t: np.zeros(tuple(t.shape), ft)      # noqa: E731
    out["grads"] = {"feats.%d" % i: (f.grad.numpy() if f.grad is not None else zero(f)) for i, f in enumerate(feats)}
    out["grads"].update({"mask_head." + k: (v.grad.numpy() if v.grad is not None else zero(v)) for k, v in W.items()})
    out["grads"].update({"conv_logits." + k: (v.grad.numpy() if v.grad is not None else zero(v)) for k, v in L.items()})
    return out


# ------------------------------------------------------------------------------------------------------------------- grids beyond the dense walk
# The kernels walk a bin's whole sample grid up to 8 per axis; beyond, only the stretch that can fall inside the map.  These boxes put the grid
# well above 8 on both axes -- 11, 54, thousands, and beyond the cut at 2^24 -- with the map at the start, in the middle and at the end of the box.
BIG_ROIS = np.array([[0, -200.0, -150.0, 400.0, 380.0], [1, -1500.0, -1400.0, 1500.0, 1600.0], [0, 3.0, 2.0, 5.0e5, 4.0e5], [1, -3.0e5, -2.0e5, 40.0, 50.0],
                     [0, -150.0, 10.0, 1100.0, 30.0], [1, -3.0e9, -3.0e9, 3.0e9, 3.0e9], [0, 1.0, 1.0, 6.0e9, 6.0e9], [1, -6.0e9, -200.0, 60.0, 400.0]], np.float32)
BIG_LEVELS = np.array([0, 0, 0, 1, 1, 0, 1, 0], np.int32)      # caller-given: the 16 x 16 and 8 x 8 maps
BIG_BITMAP_HW, BIG_BITMAP_SEED = (280, 300), 1
BIG_BOXES = np.array([[5.3, 4.1, 295.2, 270.7], [-50.0, -30.0, 400.0, 350.0], [10.2, 100.4, 290.8, 110.9], [20.0, 15.0, 280.0, 265.0]], np.float32)


def big_bitmaps(seed=BIG_BITMAP_SEED):
    """two irregular 280 x 300 bitmaps: with mask size 28 the boxes above sample them on grids of 10 and 11 per axis"""
    rng = np.random.default_rng(seed)
    H, W = BIG_BITMAP_HW
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for _ in range(2):
        m = np.zeros((H, W), bool)
        for _ in range(4):
            cy, cx, ry, rx = rng.uniform(60, 220), rng.uniform(60, 240), rng.uniform(25, 90), rng.uniform(25, 90)
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0 + 0.25 * rng.standard_normal((H, W))
        out.append(m.astype(np.uint8))
    return np.stack(out)
