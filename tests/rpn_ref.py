"""Numpy restatement of the oriented RPN (csrc/rpn.hip) for the tests of mtp_amd.dense_heads / mtp_amd.task_modules: the sibling of box_ref.py.  Plain
helper module: no tests, no fixtures.  Everything takes a `dtype`: float64 is the reference, float32 the same operations in the kernels' precision and
order -- its distance from float64 sets the tolerance of the GPU tests.
  * base_anchors / grid_priors / inside_flags: mmdet's AnchorGenerator (center_offset 0, scale_major) and anchor_inside_flags;
  * encode / decode: mmrotate's MidpointOffsetCoder, angle_version 'le90', restated from the published algorithm;
  * loss: sigmoid BCE with logits and SmoothL1 over sampled anchors, both scaled by weight / avg_factor, with the dense gradients;
  * proposals: per level the top nms_pre logits (stable), decode, size filter, NMS on the circumscribed boxes within a level, max_per_img.
Maps are NCHW arrays (N, A * C, H, W)."""
import numpy as np

import box_ref

F64, F32 = np.float64, np.float32
MAX_RATIO = abs(np.log(16 / 1000))


def base_anchors(base_size, scales, ratios):
    """the reference computes these in float32 torch; the same expressions in numpy float32 -> (A, 4) float32"""
    ratios, scales = np.asarray(ratios, F32), np.asarray(scales, F32)
    h_ratios = np.sqrt(ratios)
    w_ratios = F32(1) / h_ratios
    ws = (F32(base_size) * w_ratios[:, None] * scales[None, :]).reshape(-1)
    hs = (F32(base_size) * h_ratios[:, None] * scales[None, :]).reshape(-1)
    return np.stack([F32(-0.5) * ws, F32(-0.5) * hs, F32(0.5) * ws, F32(0.5) * hs], 1).astype(F32)


def grid_priors(base, H, W, stride, dtype=F64):
    """(H W A, 4): prior (y W + x) A + a = base[a] + (x sw, y sh, x sw, y sh)"""
    base = np.asarray(base, dtype)
    sx, sy = (np.arange(W).astype(dtype) * dtype(stride[0])), (np.arange(H).astype(dtype) * dtype(stride[1]))
    xx, yy = np.tile(sx, H), np.repeat(sy, W)
    shifts = np.stack([xx, yy, xx, yy], 1)
    return (base[None] + shifts[:, None]).reshape(-1, 4)


def inside_flags(priors, A, H, W, stride, pad_shape, img_shape, allowed_border=0):
    vw, vh = min(-(-int(pad_shape[1]) // stride[0]), W), min(-(-int(pad_shape[0]) // stride[1]), H)
    valid = ((np.arange(H) < vh)[:, None] & (np.arange(W) < vw)[None]).reshape(-1)
    valid = np.repeat(valid, A)
    if allowed_border < 0:
        return valid
    b, p = priors.dtype.type(allowed_border), priors
    return valid & (p[:, 0] >= -b) & (p[:, 1] >= -b) & (p[:, 2] < priors.dtype.type(img_shape[1]) + b) & (p[:, 3] < priors.dtype.type(img_shape[0]) + b)


def corners(g, dtype=F64):
    """(n, 4) x and (n, 4) y of ctr -+ (w/2)(cos, sin) -+ (h/2)(-sin, cos), in the kernel's order"""
    g = np.asarray(g, dtype).reshape(-1, 5)
    hw, hh, c, s = g[:, 2] * dtype(0.5), g[:, 3] * dtype(0.5), np.cos(g[:, 4]), np.sin(g[:, 4])
    ux, uy, vx, vy = hw * c, hw * s, -(hh * s), hh * c
    X = np.stack([(g[:, 0] - ux) - vx, (g[:, 0] + ux) - vx, (g[:, 0] + ux) + vx, (g[:, 0] - ux) + vx], 1)
    Y = np.stack([(g[:, 1] - uy) - vy, (g[:, 1] + uy) - vy, (g[:, 1] + uy) + vy, (g[:, 1] - uy) + vy], 1)
    return X, Y


def encode(priors, gts, means, stds, dtype=F64):
    p, g = np.asarray(priors, dtype).reshape(-1, 4), np.asarray(gts, dtype).reshape(-1, 5)
    half = dtype(0.5)
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    hb = box_ref.rbox2hbox(g, dtype)
    gx, gy, gw, gh = (hb[:, 0] + hb[:, 2]) * half, (hb[:, 1] + hb[:, 3]) * half, hb[:, 2] - hb[:, 0], hb[:, 3] - hb[:, 1]
    X, Y = corners(g, dtype)
    ymin, xmax = Y.min(1, keepdims=True), X.max(1, keepdims=True)
    ga = np.where(np.abs(Y - ymin) > dtype(0.1), dtype(-1000), X).max(1)
    gb = np.where(np.abs(X - xmax) > dtype(0.1), dtype(-1000), Y).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph), (ga - gx) / gw, (gb - gy) / gh], 1)
    return ((d - np.asarray(means, dtype)) / np.asarray(stds, dtype)).astype(dtype)


def decode(priors, deltas, means, stds, dtype=F64):
    """-> (n, 5) cx, cy, w, h, theta with w >= h, theta in [-pi/2, pi/2)"""
    p, raw = np.asarray(priors, dtype).reshape(-1, 4), np.asarray(deltas, dtype).reshape(-1, 6)
    half, pi = dtype(0.5), dtype(np.pi)
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    d = raw * np.asarray(stds, dtype) + np.asarray(means, dtype)
    mr = dtype(MAX_RATIO)
    dw, dh = np.clip(d[:, 2], -mr, mr), np.clip(d[:, 3], -mr, mr)
    gw, gh, gx, gy = pw * np.exp(dw), ph * np.exp(dh), px + pw * d[:, 0], py + ph * d[:, 1]
    da, db = np.clip(d[:, 4], -half, half), np.clip(d[:, 5], -half, half)
    c0x, c0y, c1x, c1y = da * gw, -(gh * half), gw * half, db * gh
    n0, n1 = np.sqrt(c0x * c0x + c0y * c0y), np.sqrt(c1x * c1x + c1y * c1y)
    diag = np.maximum(n0, n1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s0, s1 = np.where(n0 > 0, diag / n0, dtype(0)), np.where(n1 > 0, diag / n1, dtype(0))
    v0x, v0y, v1x, v1y = c0x * s0, c0y * s0, c1x * s1, c1y * s1
    e1x, e1y, e2x, e2y = v1x - v0x, v1y - v0y, v1x + v0x, v1y + v0y
    l1, l2 = np.sqrt(e1x * e1x + e1y * e1y), np.sqrt(e2x * e2x + e2y * e2y)
    first = l1 >= l2
    t = np.arctan2(np.where(first, e1y, e2y), np.where(first, e1x, e2x)).astype(dtype)
    t = np.where(t >= pi * half, t - pi, t)
    t = np.where(t < -(pi * half), t + pi, t)
    return np.stack([gx, gy, np.where(first, l1, l2), np.where(first, l2, l1), t], 1).astype(dtype)


def level_of(idx, sizes, A):
    """flat multi-level anchor indices -> (level, y, x, a)"""
    firsts = np.cumsum([0] + [h * w * A for h, w in sizes])
    idx = np.asarray(idx, np.int64)
    lvl = np.searchsorted(firsts, idx, side="right") - 1
    local = idx - firsts[lvl]
    W = np.asarray([w for _, w in sizes], np.int64)[lvl]
    a, cell = local % A, local // A
    return lvl, cell // W, cell % W, a


def loss(cls_maps, reg_maps, sizes, A, priors, gts_list, pos_list, pos_gt_list, neg_list, means, stds, beta, cls_weight=1.0, bbox_weight=1.0, dtype=F64,
         avg_factor=None):
    """cls_maps[l] (N, A, H, W), reg_maps[l] (N, 6 A, H, W); per image the gts (K, 5), the positive anchors with their gt rows and the negative anchors
    -> loss_cls (L), loss_bbox (L), dcls[l], dreg[l] (the gradients of the sum of all losses).  A gt row of -1 names no gt: the anchor is a positive
    for the classification and has no box term.  avg_factor: the divisor, when it is not the number of listed anchors (the kernel counts the slots
    of its lists, those whose anchor index it skips included)."""
    L = len(sizes)
    cls_maps, reg_maps = [np.asarray(m, dtype) for m in cls_maps], [np.asarray(m, dtype) for m in reg_maps]
    priors = np.asarray(priors, dtype)
    avg = sum(len(p) + len(n) for p, n in zip(pos_list, neg_list)) if avg_factor is None else int(avg_factor)
    lc, lb = [np.zeros((), dtype) for _ in range(L)], [np.zeros((), dtype) for _ in range(L)]
    dcls, dreg = [np.zeros_like(m) for m in cls_maps], [np.zeros_like(m) for m in reg_maps]
    beta = dtype(beta)
    gc = dtype(cls_weight) / dtype(avg) if avg else dtype(0)
    gb = dtype(bbox_weight) / dtype(avg) if avg else dtype(0)
    for b, (gts, pos, pgt, neg) in enumerate(zip(gts_list, pos_list, pos_gt_list, neg_list)):
        idx = np.concatenate([np.asarray(pos, np.int64), np.asarray(neg, np.int64)])
        t = np.concatenate([np.ones(len(pos), dtype), np.zeros(len(neg), dtype)])
        lvl, y, x, a = level_of(idx, sizes, A)
        tgt = encode(priors[np.asarray(pos, np.int64)], np.asarray(gts, dtype).reshape(-1, 5)[np.asarray(pgt, np.int64)], means, stds, dtype) if len(pos) else None
        for j in range(len(idx)):
            l = int(lvl[j])
            z = cls_maps[l][b, a[j], y[j], x[j]]
            lc[l] = lc[l] + ((np.maximum(z, dtype(0)) - z * t[j]) + np.log1p(np.exp(-np.abs(z))))
            dcls[l][b, a[j], y[j], x[j]] = (dtype(1) / (dtype(1) + np.exp(-z)) - t[j]) * gc
            if j < len(pos) and pgt[j] >= 0:
                ch = a[j] * 6 + np.arange(6)
                d = reg_maps[l][b, ch, y[j], x[j]] - tgt[j]
                ad = np.abs(d)
                lb[l] = lb[l] + np.where(ad < beta, (dtype(0.5) * ad) * ad / beta, ad - dtype(0.5) * beta).sum(dtype=dtype)
                dreg[l][b, ch, y[j], x[j]] = np.where(ad < beta, d / beta, np.sign(d)) * gb
    div = dtype(avg) if avg else dtype(1)
    return (np.asarray([v / div * dtype(cls_weight) for v in lc], dtype), np.asarray([v / div * dtype(bbox_weight) for v in lb], dtype), dcls, dreg)


def topk_per_level(cls_maps_b, nms_pre):
    """cls_maps_b[l] (A, H, W) of one image -> per level the kept anchor indices (y, x, a order), descending logit, stable"""
    keep = []
    for m in cls_maps_b:
        z = np.transpose(m, (1, 2, 0)).reshape(-1)
        order = np.argsort(-z, kind="stable")
        keep.append(order[:nms_pre] if 0 < nms_pre < len(z) else order)
    return keep


def decode_kept(cls_maps_b, reg_maps_b, priors, sizes, A, keep, means, stds, dtype=F64):
    """the kept anchors of one image, level after level -> scores (T), rboxes (T, 5), hboxes (T, 4), level ids (T)"""
    firsts = np.cumsum([0] + [h * w * A for h, w in sizes])
    sc, rb, ids = [], [], []
    for l, (m, r, k) in enumerate(zip(cls_maps_b, reg_maps_b, keep)):
        z = np.transpose(np.asarray(m, dtype), (1, 2, 0)).reshape(-1)[k]
        H, W = sizes[l]
        d = np.transpose(np.asarray(r, dtype).reshape(A, 6, H, W), (2, 3, 0, 1)).reshape(-1, 6)[k]
        sc.append(dtype(1) / (dtype(1) + np.exp(-z)))
        rb.append(decode(np.asarray(priors, dtype)[firsts[l] + k], d, means, stds, dtype))
        ids.append(np.full(len(k), l, np.int64))
    rb = np.concatenate(rb)
    return np.concatenate(sc).astype(dtype), rb, box_ref.rbox2hbox(rb, dtype), np.concatenate(ids)


def proposals(cls_maps_b, reg_maps_b, priors, sizes, A, means, stds, nms_pre, max_per_img, iou_threshold, min_bbox_size=0, dtype=F64):
    """one image -> (keep: positions in the concatenated kept list, in output order; rboxes (k, 5); scores (k))"""
    keep = topk_per_level(cls_maps_b, nms_pre)
    sc, rb, hb, ids = decode_kept(cls_maps_b, reg_maps_b, priors, sizes, A, keep, means, stds, dtype)
    src = np.arange(len(sc))
    if min_bbox_size >= 0:
        src = src[(rb[:, 2] > min_bbox_size) & (rb[:, 3] > min_bbox_size)]
    if len(src) == 0:
        return src, rb[src], sc[src]
    kept = src[box_ref.nms(hb[src], sc[src], iou_threshold, ids[src], dtype=dtype)][:max_per_img]
    return kept, rb[kept], sc[kept]
