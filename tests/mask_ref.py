"""numpy restatement of the mask branch (mtp_amd/csrc/mask_head.hip): mmcv's roi_align ('avg', aligned or not, fixed or adaptive grid) forward and
backward, mmdet's map_roi_levels, mask_target / crop_and_resize, mask_cross_entropy with its gradient, and _do_paste_mask + threshold.  Every
function takes `ft`, np.float64 (the reference run) or np.float32 (the yardstick: the same operations in the kernels' order, on the CPU).
Restated from the published algorithms; no GPU, no mtp_amd."""
import numpy as np

MAX_GRID = 1 << 24      # the kernels cut an adaptive grid here (a sample index beyond it is not exact in float32)


def map_roi_levels(rois, finest_scale, num_levels, ft=np.float64):
    """rois (R, 5): image, x1, y1, x2, y2 -> (R) int64; NaN -> 0"""
    r = np.asarray(rois, ft)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.floor(np.log2(np.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / ft(finest_scale) + ft(1e-6)))
    return np.where(v >= 1, np.minimum(v, num_levels - 1), 0).astype(np.int64)


def axis(a, b, scale, P, sampling, aligned, ft):
    """one axis of a RoI on a map -> (start, bin size, grid)"""
    off = ft(0.5) if aligned else ft(0.0)
    lo, hi = ft(a) * ft(scale) - off, ft(b) * ft(scale) - off
    length = hi - lo
    if not aligned:
        length = max(length, ft(1.0))
    grid = int(sampling) if sampling > 0 else (int(min(max(np.ceil(length / ft(P)), 0), MAX_GRID)) if np.isfinite(length) else 0)
    return lo, length / ft(P), grid


def sample_coord(ax, p, i, ft):
    """the coordinate of sample i of bin p, in ft, as the kernels compute it"""
    start, bin_, grid = ax
    return (start + ft(p) * bin_) + (ft(i) + ft(0.5)) * bin_ / ft(grid)


def live(ax, P, size, ft, whole=64):
    """the samples i of a bin's grid that can lie inside [-1, size] for some bin, ascending: all of them for grids up to `whole`; beyond, the union over the
    bins of [first i with v >= -1, first i with v > size), each found by bisection on the coordinate itself -- v is nondecreasing in i for a positive
    bin size in any float format (i + 0.5, the product with a positive number, the quotient by one and the sum with a constant all keep the
    order), so the samples outside the interval are exactly those the border rule gives weight 0.  Nothing of the kernels' own range arithmetic
    (margins, floor / ceil in float32) is restated here; tests/test_mask_host.py holds the bisection to a scan of every sample."""
    start, bin_, grid = ax
    if grid <= whole or not bin_ > 0:
        return range(grid)

    def first(pred, p):
        lo, hi = 0, grid
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(sample_coord(ax, p, mid, ft)):
                hi = mid
            else:
                lo = mid + 1
        return lo
    keep = set()
    for p in range(P):
        keep.update(range(first(lambda v: v >= -1, p), first(lambda v: v > size, p)))
    return sorted(keep)


def axis_samples(ax, P, i, size, ft):
    """sample i of every bin 0 .. P - 1 -> (ok (P) bool, lo, hi (P) int64, weight of lo, weight of hi (P) ft); mmcv's bilinear_interpolate, one axis"""
    start, bin_, grid = ax
    p = np.arange(P).astype(ft)
    with np.errstate(invalid="ignore"):
        v = (start + p * bin_) + (ft(i) + ft(0.5)) * bin_ / ft(grid)
        ok = (v >= -1) & (v <= size)
    v = np.where(ok, np.maximum(v, 0), 0).astype(ft)
    lo = v.astype(np.int64)
    edge = lo >= size - 1
    lo = np.where(edge, size - 1, lo)
    hi = np.where(edge, size - 1, lo + 1)
    v = np.where(edge, lo.astype(ft), v)
    wh = (v - lo.astype(ft)).astype(ft)
    return ok, lo, hi, (ft(1.0) - wh).astype(ft), wh


def count_of(ay, ax, ft):
    return max(ft(ay[2]) * ft(ax[2]), ft(1.0))


def roi_align(maps, rois, strides, P, sampling, aligned, finest_scale, levels=None, in_use=None, ft=np.float64):
    """maps: per level (N, C, H, W); rois (R, 5) -> (out (R, C, P, P) ft, levels (R) int64).  Per bin the samples are added in the kernel's order:
    iy outer, ix inner, each sample as ((w1 v1 + w2 v2) + w3 v3) + w4 v4, then / count.  in_use (R) bool: the other slots give zeros."""
    rois = np.asarray(rois)
    R, C = len(rois), maps[0].shape[1]
    lv = map_roi_levels(rois, finest_scale, len(maps), ft) if levels is None else np.clip(np.asarray(levels, np.int64), 0, len(maps) - 1)
    out = np.zeros((R, C, P, P), ft)
    for r in range(R):
        b = rois[r, 0]
        if not (0 <= b < maps[0].shape[0]) or (in_use is not None and not in_use[r]):
            continue
        m = np.asarray(maps[lv[r]][int(b)], ft)
        H, W = m.shape[1:]
        s = 1.0 / strides[lv[r]]
        ay, ax = axis(rois[r, 2], rois[r, 4], s, P, sampling, aligned, ft), axis(rois[r, 1], rois[r, 3], s, P, sampling, aligned, ft)
        acc = np.zeros((C, P, P), ft)
        xs = live(ax, P, W, ft)
        for iy in live(ay, P, H, ft):
            oky, yl, yh, hy, ly = axis_samples(ay, P, iy, H, ft)
            if not oky.any():
                continue
            for ix in xs:
                okx, xl, xh, hx, lx = axis_samples(ax, P, ix, W, ft)
                v1, v2 = m[:, yl[:, None], xl[None, :]], m[:, yl[:, None], xh[None, :]]
                v3, v4 = m[:, yh[:, None], xl[None, :]], m[:, yh[:, None], xh[None, :]]
                val = (((hy[:, None] * hx[None, :]) * v1 + (hy[:, None] * lx[None, :]) * v2) + (ly[:, None] * hx[None, :]) * v3) + (ly[:, None] * lx[None, :]) * v4
                acc += np.where(oky[:, None] & okx[None, :], val, 0).astype(ft)
        out[r] = acc / count_of(ay, ax, ft)
    return out, lv


def axis_weights(ax, P, size, ft):
    """(P, size): the weight the samples of bin p put on pixel q of this axis, added sample after sample"""
    w = np.zeros((P, size), ft)
    p = np.arange(P)
    for i in live(ax, P, size, ft):
        ok, lo, hi, wl, wh = axis_samples(ax, P, i, size, ft)
        w[p[ok], lo[ok]] += wl[ok]
        w[p[ok], hi[ok]] += wh[ok]
    return w


def roi_align_bwd(dout, shapes, rois, strides, P, sampling, aligned, finest_scale, levels=None, in_use=None, ft=np.float64):
    """dout (R, C, P, P); shapes: per level (N, C, H, W) -> per level the gradient (N, C, H, W) ft.  The kernel's separable form and order: per
    pixel the RoIs in index order, bins i then j, acc += (Wy[i] Wx[j]) (dout[i, j] / count)."""
    rois = np.asarray(rois)
    lv = map_roi_levels(rois, finest_scale, len(shapes), ft) if levels is None else np.clip(np.asarray(levels, np.int64), 0, len(shapes) - 1)
    grads = [np.zeros(s, ft) for s in shapes]
    d = np.asarray(dout, ft)
    for r in range(len(rois)):
        b = rois[r, 0]
        if not (0 <= b < shapes[0][0]) or (in_use is not None and not in_use[r]):
            continue
        g = grads[lv[r]][int(b)]
        H, W = g.shape[1:]
        s = 1.0 / strides[lv[r]]
        ay, ax = axis(rois[r, 2], rois[r, 4], s, P, sampling, aligned, ft), axis(rois[r, 1], rois[r, 3], s, P, sampling, aligned, ft)
        wy, wx = axis_weights(ay, P, H, ft), axis_weights(ax, P, W, ft)
        cnt = count_of(ay, ax, ft)
        ys, xs = np.nonzero(wy.any(0))[0], np.nonzero(wx.any(0))[0]
        if not len(ys) or not len(xs):
            continue
        sub = g[:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        wy, wx = wy[:, ys[0]:ys[-1] + 1], wx[:, xs[0]:xs[-1] + 1]
        for i in range(P):
            if not wy[i].any():
                continue
            for j in range(P):
                if not wx[j].any():
                    continue
                sub += ((wy[i][:, None] * wx[j][None, :]).astype(ft)[None] * (d[r, :, i, j] / cnt).astype(ft)[:, None, None]).astype(ft)
    return grads


def mask_targets(boxes, gt_rows, bitmaps, M, img_hw=None, ft=np.float64):
    """mmdet's mask_target_single + BitmapMasks.crop_and_resize: boxes (n, 4) clipped to the image, bitmaps[gt_rows[i]] sampled at M x M by
    roi_align(aligned, adaptive grid, scale 1) -> (avg (n, M, M) ft, targets (n, M, M) uint8 = avg >= 0.5)"""
    boxes = np.asarray(boxes, ft)
    n = len(boxes)
    avg = np.zeros((n, M, M), ft)
    for i in range(n):
        bm = np.asarray(bitmaps[gt_rows[i]])
        h, w = bm.shape if img_hw is None else img_hw[i]
        x1, x2 = np.clip(boxes[i, [0, 2]], 0, w)
        y1, y2 = np.clip(boxes[i, [1, 3]], 0, h)
        roi = np.array([[0, x1, y1, x2, y2]], ft)
        avg[i] = roi_align([bm[None, None, :h, :w].astype(ft)], roi, [1], M, 0, True, 56.0, levels=[0], ft=ft)[0][0, 0]
    return avg, (avg >= 0.5).astype(np.uint8)


def sigmoid(z, ft):
    z = np.asarray(z, ft)
    en = np.exp(-np.abs(z)).astype(ft)
    return np.where(z >= 0, ft(1.0) / (ft(1.0) + en), en / (ft(1.0) + en)).astype(ft)


def mask_loss(logits, targets, channels, n_total, loss_weight=1.0, ft=np.float64):
    """mmdet's mask_cross_entropy over fixed slots: logits (R, K, M, M); targets (R, M, M) 0 / 1; channels (R): the class channel of a positive
    slot, -1 for padding; n_total positives -> (loss, slot sums (R), dlogits (R, K, M, M)).  mean over n_total M M, times loss_weight; without a
    positive everything is 0."""
    z = np.asarray(logits, ft)
    R, K, M, _ = z.shape
    d = np.zeros(z.shape, ft)
    slot = np.zeros(R, ft)
    scale = ft(loss_weight) / (ft(n_total) * ft(M * M)) if n_total > 0 else ft(0.0)
    for r in range(R):
        k = int(channels[r])
        if k < 0:
            continue
        t = np.asarray(targets[r], ft)
        zz = z[r, k]
        slot[r] = ((np.maximum(zz, 0) - zz * t) + np.log1p(np.exp(-np.abs(zz)))).astype(ft).sum(dtype=ft)
        d[r, k] = (sigmoid(zz, ft) - t) * scale
    loss = slot.sum(dtype=ft) / (ft(n_total) * ft(M * M)) * ft(loss_weight) if n_total > 0 else ft(0.0)
    return ft(loss), slot, d


def paste(logits, labels, boxes, img_h, img_w, threshold, activate=True, ft=np.float64):
    """_do_paste_mask(skip_empty=False) + threshold: logits (N, K, M, M), labels (N) or None (channel 0), boxes (N, 4) -> (values (N, img_h, img_w)
    ft, masks: bool = values >= threshold, or uint8 = values * 255 truncated when threshold < 0).  grid_sample bilinear, zeros padding,
    align_corners=False; an infinite normalised coordinate is 0."""
    z = np.asarray(logits, ft)
    N, K, M, _ = z.shape
    boxes = np.asarray(boxes, ft)
    vals = np.zeros((N, img_h, img_w), ft)

    def coord(n_pix, a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            g = ((np.arange(n_pix).astype(ft) + ft(0.5)) - a) / (b - a) * ft(2.0) - ft(1.0)
        g = np.where(np.isinf(g), ft(0.0), g).astype(ft)
        return (((g + ft(1.0)) * ft(M) - ft(1.0)) / ft(2.0)).astype(ft)

    for n in range(N):
        k = 0 if labels is None else int(labels[n])
        m = sigmoid(z[n, k], ft) if activate else z[n, k]
        sx, sy = coord(img_w, boxes[n, 0], boxes[n, 2]), coord(img_h, boxes[n, 1], boxes[n, 3])
        nan = np.isnan(sy)[:, None] | np.isnan(sx)[None, :]
        sx0, sy0 = np.where(np.isnan(sx), ft(0.0), sx), np.where(np.isnan(sy), ft(0.0), sy)
        fx, fy = np.floor(sx0), np.floor(sy0)
        wx1, wx0, wy1, wy0 = (sx0 - fx).astype(ft), ((fx + ft(1.0)) - sx0).astype(ft), (sy0 - fy).astype(ft), ((fy + ft(1.0)) - sy0).astype(ft)
        x0, y0 = np.clip(fx, -2, M + 1).astype(np.int64), np.clip(fy, -2, M + 1).astype(np.int64)

        def corner(dy, dx):
            cy, cx = y0 + dy, x0 + dx
            inside = ((cy >= 0) & (cy < M))[:, None] & ((cx >= 0) & (cx < M))[None, :]
            return np.where(inside, m[np.clip(cy, 0, M - 1)[:, None], np.clip(cx, 0, M - 1)[None, :]], ft(0.0)).astype(ft)

        v = ((corner(0, 0) * (wy0[:, None] * wx0[None, :]) + corner(0, 1) * (wy0[:, None] * wx1[None, :])) + corner(1, 0) * (wy1[:, None] * wx0[None, :])) \
            + corner(1, 1) * (wy1[:, None] * wx1[None, :])
        vals[n] = np.where(nan, np.nan, v)
    if threshold >= 0:
        with np.errstate(invalid="ignore"):
            return vals, vals >= threshold
    return vals, np.where(np.isnan(vals), 0, np.clip(vals * ft(255.0), 0, 255)).astype(np.uint8)
