"""Numpy restatement of the oriented RoI head (csrc/roi_head.hip) for the tests of mtp_amd.ops_roi / roi_extractors / roi_heads: the sibling of
rpn_ref.py.  Plain helper module: no tests, no fixtures.  Everything takes a `dtype`: float64 is the reference, float32 the same operations in the
kernels' precision and order -- its distance from float64 sets the tolerance of the GPU tests.
  * map_levels: mmdet's SingleRoIExtractor.map_roi_levels;
  * sample_points / roi_align / roi_align_bwd: mmcv's roi_align_rotated with aligned=True, restated from the published algorithm;
  * encode / decode: mmrotate's DeltaXYWHTRBBoxCoder, 'le90', edge_swap, proj_xy, norm_factor None;
  * loss: softmax cross-entropy and SmoothL1 over the sampled RoIs with their dense gradients, top-1 accuracy;
  * predict: softmax scores, decoded boxes, the (roi, class) candidates above score_thr, nms_rotated within a class, max_per_img.
Maps are NCHW arrays (N, C, H, W); RoIs are (R, 6) = image, cx, cy, w, h, theta; RoI features are (R, C, P, P) as mmcv has them."""
import numpy as np

import box_ref

F64, F32 = np.float64, np.float32
MAX_RATIO = abs(np.log(16 / 1000))


def map_levels(rois, num_levels, finest_scale=56, dtype=F64):
    r = np.asarray(rois, dtype).reshape(-1, 6)
    with np.errstate(divide="ignore"):
        v = np.floor(np.log2(np.sqrt(r[:, 3] * r[:, 4]) / dtype(finest_scale) + dtype(1e-6)))
    return np.clip(v, 0, num_levels - 1).astype(np.int64)


def level_margin(rois, finest_scale=56):
    """distance of log2(sqrt(w h) / finest_scale) from the nearest integer"""
    r = np.asarray(rois, F64).reshape(-1, 6)
    v = np.log2(np.sqrt(r[:, 3] * r[:, 4]) / finest_scale + 1e-6)
    return np.abs(v - np.round(v))


def sample_points(roi, H, W, scale, P, S, clockwise, dtype=F64):
    """one RoI on one level -> y, x (P P, S S) the sample coordinates before the bilinear rules, in the kernel's order of operations"""
    roi = np.asarray(roi, dtype)
    scale, half = dtype(scale), dtype(0.5)
    cx, cy, rw, rh = roi[1] * scale - half, roi[2] * scale - half, roi[3] * scale, roi[4] * scale
    th = -roi[5] if clockwise else roi[5]
    cs, sn = np.cos(th), np.sin(th)
    bh, bw = rh / dtype(P), rw / dtype(P)
    b, s = np.arange(P * P)[:, None], np.arange(S * S)[None, :]
    ph, pw, iy, ix = (b // P).astype(dtype), (b % P).astype(dtype), (s // S).astype(dtype), (s % S).astype(dtype)
    yy = (-rh / dtype(2) + ph * bh) + (iy + half) * bh / dtype(S)
    xx = (-rw / dtype(2) + pw * bw) + (ix + half) * bw / dtype(S)
    return ((yy * cs - xx * sn) + cy).astype(dtype), ((yy * sn + xx * cs) + cx).astype(dtype)


def bilinear(y, x, H, W, dtype=F64):
    """-> inside (bool), (yl, yh, xl, xh) int64, (w1, w2, w3, w4) for the corners (yl, xl), (yl, xh), (yh, xl), (yh, xh): mmcv's rules"""
    y, x = np.asarray(y, dtype).copy(), np.asarray(x, dtype).copy()
    inside = (y >= -1) & (y <= H) & (x >= -1) & (x <= W)
    y, x = np.where(inside, y, 0), np.where(inside, x, 0)
    y, x = np.where(y <= 0, dtype(0), y), np.where(x <= 0, dtype(0), x)
    yl, xl = y.astype(np.int64), x.astype(np.int64)
    ytop, xtop = yl >= H - 1, xl >= W - 1
    yl, xl = np.where(ytop, H - 1, yl), np.where(xtop, W - 1, xl)
    yh, xh = np.where(ytop, H - 1, yl + 1), np.where(xtop, W - 1, xl + 1)
    y, x = np.where(ytop, yl.astype(dtype), y), np.where(xtop, xl.astype(dtype), x)
    ly, lx = (y - yl.astype(dtype)).astype(dtype), (x - xl.astype(dtype)).astype(dtype)
    hy, hx = dtype(1) - ly, dtype(1) - lx
    return inside, (yl, yh, xl, xh), (hy * hx, hy * lx, ly * hx, ly * lx)


def cutoff_margin(rois, levels, sizes, strides, P, S, clockwise):
    """the smallest distance of any sample coordinate from the zero cut-offs -1, H, W (float64)"""
    m = np.inf
    for roi, l in zip(np.asarray(rois, F64).reshape(-1, 6), levels):
        H, W = sizes[l]
        y, x = sample_points(roi, H, W, 1.0 / strides[l], P, S, clockwise)
        m = min(m, np.abs(y + 1).min(), np.abs(y - H).min(), np.abs(x + 1).min(), np.abs(x - W).min())
    return m


def roi_align(maps, rois, strides, P=7, S=2, clockwise=False, finest_scale=56, levels=None, valid=None, dtype=F64):
    """maps[l] (N, C, H, W) -> (R, C, P, P); valid (R) bool: a slot that is not in use gives zeros"""
    maps = [np.asarray(m, dtype) for m in maps]
    rois = np.asarray(rois, dtype).reshape(-1, 6)
    levels = map_levels(rois, len(maps), finest_scale, dtype) if levels is None else np.asarray(levels)
    R, C = len(rois), maps[0].shape[1]
    out = np.zeros((R, C, P * P), dtype)
    count = dtype(max(S * S, 1))
    for r in range(R):
        if valid is not None and not valid[r]:
            continue
        m = maps[levels[r]]
        H, W = m.shape[2:]
        y, x = sample_points(rois[r], H, W, 1.0 / strides[levels[r]], P, S, clockwise, dtype)
        inside, (yl, yh, xl, xh), w = bilinear(y, x, H, W, dtype)
        f = m[int(rois[r, 0])]
        acc = np.zeros((C, P * P), dtype)
        for s in range(S * S):
            val = ((w[0][:, s] * f[:, yl[:, s], xl[:, s]] + w[1][:, s] * f[:, yl[:, s], xh[:, s]]) + w[2][:, s] * f[:, yh[:, s], xl[:, s]]) \
                + w[3][:, s] * f[:, yh[:, s], xh[:, s]]
            acc = acc + np.where(inside[:, s], val, dtype(0))
        out[r] = acc / count
    return out.reshape(R, C, P, P)


def roi_align_one(m, roi, stride, P, S, clockwise):
    """brute force, float64, one RoI on one map (C, H, W): four nested loops and scalar arithmetic, written from the definition alone"""
    C, H, W = m.shape
    scale = 1.0 / stride
    cx, cy, rw, rh = roi[1] * scale - 0.5, roi[2] * scale - 0.5, roi[3] * scale, roi[4] * scale
    th = -roi[5] if clockwise else roi[5]
    out = np.zeros((C, P, P))
    for ph in range(P):
        for pw in range(P):
            for iy in range(S):
                for ix in range(S):
                    yy = -rh / 2 + (ph + (iy + 0.5) / S) * rh / P
                    xx = -rw / 2 + (pw + (ix + 0.5) / S) * rw / P
                    y, x = yy * np.cos(th) - xx * np.sin(th) + cy, yy * np.sin(th) + xx * np.cos(th) + cx
                    if y < -1 or y > H or x < -1 or x > W:
                        continue
                    y, x = max(y, 0.0), max(x, 0.0)
                    y0, x0 = int(y), int(x)
                    if y0 >= H - 1:
                        y0 = y1 = H - 1
                        y = float(y0)
                    else:
                        y1 = y0 + 1
                    if x0 >= W - 1:
                        x0 = x1 = W - 1
                        x = float(x0)
                    else:
                        x1 = x0 + 1
                    ly, lx = y - y0, x - x0
                    out[:, ph, pw] += ((1 - ly) * (1 - lx) * m[:, y0, x0] + (1 - ly) * lx * m[:, y0, x1] + ly * (1 - lx) * m[:, y1, x0] + ly * lx * m[:, y1, x1])
    return out / (S * S)


def roi_align_bwd(dout, shapes, rois, strides, P=7, S=2, clockwise=False, finest_scale=56, levels=None, valid=None, dtype=F64):
    """dout (R, C, P, P), shapes[l] = (N, C, H, W) -> the gradients of the maps.  (The order of additions into one pixel is not the kernel's sorted
    order; the float32 run still measures the size of the rounding.)"""
    dout = np.asarray(dout, dtype)
    rois = np.asarray(rois, dtype).reshape(-1, 6)
    levels = map_levels(rois, len(shapes), finest_scale, dtype) if levels is None else np.asarray(levels)
    grads = [np.zeros(s, dtype) for s in shapes]
    count = dtype(max(S * S, 1))
    R, C = dout.shape[:2]
    d = dout.reshape(R, C, P * P)
    for r in range(R):
        if valid is not None and not valid[r]:
            continue
        g = grads[levels[r]]
        H, W = g.shape[2:]
        y, x = sample_points(rois[r], H, W, 1.0 / strides[levels[r]], P, S, clockwise, dtype)
        inside, (yl, yh, xl, xh), w = bilinear(y, x, H, W, dtype)
        b = int(rois[r, 0])
        for bin_ in range(P * P):
            for s in range(S * S):
                if not inside[bin_, s]:
                    continue
                for k, (yy, xx) in enumerate(((yl, xl), (yl, xh), (yh, xl), (yh, xh))):
                    g[b, :, yy[bin_, s], xx[bin_, s]] += (w[k][bin_, s] / count) * d[r, :, bin_]
    return grads


# ------------------------------------------------------------------------------------------------------------------- the coder
def norm_angle(a, dtype=F64):
    pi = dtype(np.pi)
    t = a + pi * dtype(0.5)
    return ((t - np.floor(t / pi) * pi) - pi * dtype(0.5)).astype(dtype)


def angle_margins(priors, gts):
    """float64: (| |d1| - |d2| |, distance of the chosen delta from the wrap of norm_angle).  Of d1 and d2 = norm(d1 + pi/2) the one of smaller
    magnitude is chosen, so it stays pi/4 clear of the wrap; the other may sit on it (a gt against itself: d2 = -+pi/2), where only its magnitude is
    read, and that is pi/2 on either side."""
    p, g = np.asarray(priors, F64).reshape(-1, 5), np.asarray(gts, F64).reshape(-1, 5)
    d = g[:, 4] - p[:, 4]
    d1, d2 = norm_angle(d), norm_angle(d + np.pi / 2)
    chosen = np.where(np.abs(d1) < np.abs(d2), d1, d2)
    return np.abs(np.abs(d1) - np.abs(d2)), np.pi / 2 - np.abs(chosen)


def encode(priors, gts, means, stds, dtype=F64):
    p, g = np.asarray(priors, dtype).reshape(-1, 5), np.asarray(gts, dtype).reshape(-1, 5)
    cs, sn = np.cos(p[:, 4]), np.sin(p[:, 4])
    ex, ey = g[:, 0] - p[:, 0], g[:, 1] - p[:, 1]
    dx, dy = (cs * ex + sn * ey) / p[:, 2], (-sn * ex + cs * ey) / p[:, 3]
    half_pi = dtype(np.pi) * dtype(0.5)
    d1, d2 = norm_angle(g[:, 4] - p[:, 4], dtype), norm_angle((g[:, 4] - p[:, 4]) + half_pi, dtype)
    first = np.abs(d1) < np.abs(d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        dw, dh = np.log(np.where(first, g[:, 2], g[:, 3]) / p[:, 2]), np.log(np.where(first, g[:, 3], g[:, 2]) / p[:, 3])
    d = np.stack([dx, dy, dw, dh, np.where(first, d1, d2)], 1)
    return ((d - np.asarray(means, dtype)) / np.asarray(stds, dtype)).astype(dtype)


def decode(priors, deltas, means, stds, dtype=F64, swapped=False):
    """-> (n, 5) cx, cy, w, h, theta with w >= h, theta in [-pi/2, pi/2) (and, when swapped, gw, gh and the angle before the edge swap)"""
    p, raw = np.asarray(priors, dtype).reshape(-1, 5), np.asarray(deltas, dtype).reshape(-1, 5)
    d = raw * np.asarray(stds, dtype) + np.asarray(means, dtype)
    mr = dtype(MAX_RATIO)
    dw, dh = np.clip(d[:, 2], -mr, mr), np.clip(d[:, 3], -mr, mr)
    cs, sn = np.cos(p[:, 4]), np.sin(p[:, 4])
    gx = ((d[:, 0] * p[:, 2]) * cs - (d[:, 1] * p[:, 3]) * sn) + p[:, 0]
    gy = ((d[:, 0] * p[:, 2]) * sn + (d[:, 1] * p[:, 3]) * cs) + p[:, 1]
    gw, gh, ga = p[:, 2] * np.exp(dw), p[:, 3] * np.exp(dh), norm_angle(p[:, 4] + d[:, 4], dtype)
    keep = gw > gh
    t = norm_angle(np.where(keep, ga, ga + dtype(np.pi) * dtype(0.5)), dtype)
    out = np.stack([gx, gy, np.where(keep, gw, gh), np.where(keep, gh, gw), t], 1).astype(dtype)
    return (out, gw, gh, ga) if swapped else out


# ------------------------------------------------------------------------------------------------------------------- loss
def loss(cls_score, bbox_pred, K, rois, gts, gt_labels, sample_gt, n_pos, n_neg, means, stds, beta=1.0, cls_weight=1.0, bbox_weight=1.0, dtype=F64):
    """cls_score (B S, K + 1), bbox_pred (B S, 5), rois (B S, 5); sample_gt (B, S) rows of gts; n_pos, n_neg (B)
    -> dict(loss_cls, loss_bbox, acc, dcls, dreg, labels (B S; -1 on padding), targets (B S, 5))"""
    z, reg = np.asarray(cls_score, dtype), np.asarray(bbox_pred, dtype)
    B, S = np.asarray(sample_gt).shape
    total = int(np.sum(n_pos) + np.sum(n_neg))
    gc = dtype(cls_weight) / dtype(max(total, 1))
    gb = dtype(bbox_weight) / dtype(total) if total else dtype(0)
    beta = dtype(beta)
    dcls, dreg = np.zeros_like(z), np.zeros_like(reg)
    labels, targets = -np.ones(B * S, np.int64), np.zeros((B * S, 5), dtype)
    lc = lb = dtype(0)
    hits = 0
    for b in range(B):
        for j in range(int(n_pos[b] + n_neg[b])):
            r = b * S + j
            pos = j < n_pos[b]
            label = int(gt_labels[sample_gt[b, j]]) if pos else K
            labels[r] = label
            m = z[r].max()
            e = np.exp(z[r] - m)
            s = e.sum(dtype=dtype)
            lc = lc + ((np.log(s) + m) - z[r, label])
            hits += int(np.argmax(z[r]) == label)
            onehot = np.zeros(K + 1, dtype)
            onehot[label] = 1
            dcls[r] = (e / s - onehot) * gc
            if pos:
                t = encode(np.asarray(rois, dtype)[r], np.asarray(gts, dtype)[sample_gt[b, j]], means, stds, dtype)[0]
                targets[r] = t
                d = reg[r] - t
                ad = np.abs(d)
                lb = lb + np.where(ad < beta, (dtype(0.5) * ad) * ad / beta, ad - dtype(0.5) * beta).sum(dtype=dtype)
                dreg[r] = np.where(ad < beta, d / beta, np.sign(d)) * gb
    return dict(loss_cls=dtype(lc / dtype(max(total, 1)) * dtype(cls_weight)), loss_bbox=dtype(lb / dtype(total) * dtype(bbox_weight)) if total else dtype(0),
                acc=dtype(hits * 100.0 / total) if total else dtype(0), dcls=dcls, dreg=dreg, labels=labels, targets=targets)


def top1_margin(cls_score, rows):
    z = np.sort(np.asarray(cls_score, F64)[rows], 1)
    return (z[:, -1] - z[:, -2]).min() if len(z) else np.inf


# ------------------------------------------------------------------------------------------------------------------- the layers
def fc_forward(x, W, dtype=F64, rnd=None):
    """x (R, C P P) in the reference's flatten order (c, ph, pw); W: shared_fcs.0/1 and fc_cls / fc_reg weights and biases.  rnd: a rounding applied
    to every GEMM operand and to the outputs of the two shared layers (the bf16 engine), or None -> (cls_score, bbox_pred, context)"""
    r = (lambda a: a) if rnd is None else (lambda a: rnd(np.asarray(a, dtype)).astype(dtype))
    w = {k: np.asarray(v, dtype) for k, v in W.items()}
    x = r(np.asarray(x, dtype))
    z1 = r(x @ r(w["shared_fcs.0.weight"]).T + w["shared_fcs.0.bias"])
    y1 = np.maximum(z1, 0)
    z2 = r(y1 @ r(w["shared_fcs.1.weight"]).T + w["shared_fcs.1.bias"])
    y2 = np.maximum(z2, 0)
    cls = y2 @ r(w["fc_cls.weight"]).T + w["fc_cls.bias"]
    reg = y2 @ r(w["fc_reg.weight"]).T + w["fc_reg.bias"]
    return cls.astype(dtype), reg.astype(dtype), dict(x=x, z1=z1, y1=y1, z2=z2, y2=y2, w=w, r=r)


def fc_backward(dcls, dreg, c, dtype=F64):
    """-> ({parameter: gradient}, dx (R, C P P))"""
    r, w = c["r"], c["w"]
    dcls, dreg = r(np.asarray(dcls, dtype)), r(np.asarray(dreg, dtype))
    G = {"fc_cls.weight": dcls.T @ c["y2"], "fc_cls.bias": dcls.sum(0), "fc_reg.weight": dreg.T @ c["y2"], "fc_reg.bias": dreg.sum(0)}
    dz2 = r((dcls @ r(w["fc_cls.weight"]) + dreg @ r(w["fc_reg.weight"])) * (c["z2"] > 0))
    G["shared_fcs.1.weight"], G["shared_fcs.1.bias"] = dz2.T @ c["y1"], dz2.sum(0)
    dz1 = r((dz2 @ r(w["shared_fcs.1.weight"])) * (c["z1"] > 0))
    G["shared_fcs.0.weight"], G["shared_fcs.0.bias"] = dz1.T @ c["x"], dz1.sum(0)
    return {k: v.astype(dtype) for k, v in G.items()}, (dz1 @ r(w["shared_fcs.0.weight"])).astype(dtype)


# ------------------------------------------------------------------------------------------------------------------- predict
def softmax(z, dtype=F64):
    z = np.asarray(z, dtype)
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True, dtype=dtype)).astype(dtype)


def predict(cls_score, bbox_pred, K, rois, means, stds, score_thr, iou_threshold, max_per_img, dtype=F64):
    """one image: cls_score (R, K + 1), bbox_pred (R, 5), rois (R, 5) -> (keep: (roi, class) candidates as roi * K + class, descending score;
    boxes (k, 5); scores (k); labels (k)), and the whole score table and boxes"""
    sc = softmax(cls_score, dtype)[:, :K]
    boxes = decode(rois, bbox_pred, means, stds, dtype)
    flat = sc.reshape(-1)
    cand = np.nonzero(flat > dtype(score_thr))[0]
    if len(cand) == 0:
        return cand, boxes[:0], flat[:0], cand, sc, boxes
    kept = cand[box_ref.nms(boxes[cand // K], flat[cand], iou_threshold, cand % K, rotated=True, dtype=dtype)]
    if max_per_img > 0:
        kept = kept[:max_per_img]
    return kept, boxes[kept // K], flat[kept], kept % K, sc, boxes
