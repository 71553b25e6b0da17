"""Numpy restatement of the box operators behind the two detection families, for the tests of mtp_amd.ops_box / mtp_amd.task_modules (the sibling of
seg_eval_ref.py).  Plain helper module: no tests, no fixtures.  Everything takes a `dtype`: float64 is the reference, float32 is the same operations
in the kernels' precision -- its distance from float64 sets the tolerance of the GPU tests.
  * bbox_overlaps: mmdet's semantics (x1, y1, x2, y2; no +1; union = max(a1 + a2 - inter, eps); 'iof' divides by max(a1, eps));
  * box_iou_rotated: mmcv's semantics (cx, cy, w, h, theta; 0 when an area is below 1e-14), the intersection by convex clipping: box A is moved into
    B's frame (centres translated to B's centre first) and clipped against B's four axis-parallel half planes (Sutherland-Hodgman), shoelace area;
  * rbox2hbox: the circumscribed box, half extents |w/2 cos| + |h/2 sin| and |w/2 sin| + |h/2 cos|;
  * nms: greedy, sequential, stable order (among equal scores the lower index first), group ids (a pair suppresses only within one group);
  * assign: MaxIoUAssigner.assign_wrt_overlaps (rotated_detection/max_iou_assigner.py:231-314), pinned against the reference's own runs by f21.
"""
import numpy as np

F64, F32 = np.float64, np.float32
MAXV = 8      # a rectangle clipped by four half planes has at most 8 vertices


def bbox_overlaps(b1, b2, mode="iou", is_aligned=False, eps=1e-6, dtype=F64):
    b1, b2 = np.asarray(b1, dtype).reshape(-1, 4), np.asarray(b2, dtype).reshape(-1, 4)
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    if not is_aligned:
        b1, b2, a1, a2 = b1[:, None], b2[None], a1[:, None], a2[None]
    w = np.maximum(np.minimum(b1[..., 2], b2[..., 2]) - np.maximum(b1[..., 0], b2[..., 0]), dtype(0))
    h = np.maximum(np.minimum(b1[..., 3], b2[..., 3]) - np.maximum(b1[..., 1], b2[..., 1]), dtype(0))
    inter = w * h
    base = (a1 + a2) - inter if mode == "iou" else a1 + np.zeros_like(inter)
    return inter / np.maximum(base, dtype(eps))


def rbox2hbox(r, dtype=F64):
    r = np.asarray(r, dtype).reshape(-1, 5)
    hw, hh, c, s = r[:, 2] * dtype(0.5), r[:, 3] * dtype(0.5), np.cos(r[:, 4]), np.sin(r[:, 4])
    ex, ey = np.abs(hw * c) + np.abs(hh * s), np.abs(hw * s) + np.abs(hh * c)
    return np.stack([r[:, 0] - ex, r[:, 1] - ey, r[:, 0] + ex, r[:, 1] + ey], 1)


def _clip(px, py, n, axis, sign, bound):
    """one Sutherland-Hodgman pass over P polygons at once: keep sign * coordinate[axis] <= bound"""
    P = px.shape[0]
    ox, oy, m = np.zeros_like(px), np.zeros_like(py), np.zeros(P, np.int64)
    rows = np.arange(P)
    sgn = px.dtype.type(sign)
    for i in range(MAXV):
        act = i < n
        j = np.where(i + 1 < n, i + 1, 0)
        ax, ay, bx, by = px[:, i], py[:, i], px[rows, j], py[rows, j]
        dp = sgn * (ay if axis else ax) - bound
        dq = sgn * (by if axis else bx) - bound
        pin, qin = dp <= 0, dq <= 0
        e = act & pin & (m < MAXV)
        ox[rows[e], m[e]], oy[rows[e], m[e]] = ax[e], ay[e]
        m = m + e
        e = act & (pin != qin) & (m < MAXV)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = dp / (dp - dq)
            x, y = ax + t * (bx - ax), ay + t * (by - ay)
        if axis:
            y = sgn * bound
        else:
            x = sgn * bound
        ox[rows[e], m[e]], oy[rows[e], m[e]] = x[e], y[e]
        m = m + e
    return ox, oy, m


def _rot_pairs(a, b, mode, dtype):
    """aligned rotated IoU of P pairs (P, 5) x (P, 5)"""
    P = a.shape[0]
    ahw, ahh, ac, asn, aarea = a[:, 2] * dtype(0.5), a[:, 3] * dtype(0.5), np.cos(a[:, 4]), np.sin(a[:, 4]), a[:, 2] * a[:, 3]
    bhw, bhh, bc, bsn, barea = b[:, 2] * dtype(0.5), b[:, 3] * dtype(0.5), np.cos(b[:, 4]), np.sin(b[:, 4]), b[:, 2] * b[:, 3]
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    ox, oy = dx * bc + dy * bsn, dy * bc - dx * bsn
    cp, sp = ac * bc + asn * bsn, asn * bc - ac * bsn
    ux, uy, vx, vy = ahw * cp, ahw * sp, -(ahh * sp), ahh * cp
    px, py = np.zeros((P, MAXV), dtype), np.zeros((P, MAXV), dtype)
    px[:, 0], py[:, 0] = (ox - ux) - vx, (oy - uy) - vy
    px[:, 1], py[:, 1] = (ox + ux) - vx, (oy + uy) - vy
    px[:, 2], py[:, 2] = (ox + ux) + vx, (oy + uy) + vy
    px[:, 3], py[:, 3] = (ox - ux) + vx, (oy - uy) + vy
    n = np.full(P, 4, np.int64)
    px, py, n = _clip(px, py, n, 0, 1, bhw)
    px, py, n = _clip(px, py, n, 0, -1, bhw)
    px, py, n = _clip(px, py, n, 1, 1, bhh)
    px, py, n = _clip(px, py, n, 1, -1, bhh)
    rows, acc = np.arange(P), np.zeros(P, dtype)
    for i in range(MAXV):
        j = np.where(i + 1 < n, i + 1, 0)
        term = px[:, i] * py[rows, j] - px[rows, j] * py[:, i]
        acc = np.where(i < n, acc + term, acc)
    inter = dtype(0.5) * np.abs(acc)
    base = (aarea + barea) - inter if mode == "iou" else aarea
    with np.errstate(divide="ignore", invalid="ignore"):
        out = inter / base
    return np.where((aarea < dtype(1e-14)) | (barea < dtype(1e-14)), dtype(0), out).astype(dtype)


def box_iou_rotated(b1, b2, mode="iou", aligned=False, dtype=F64):
    b1, b2 = np.asarray(b1, dtype).reshape(-1, 5), np.asarray(b2, dtype).reshape(-1, 5)
    if aligned:
        return _rot_pairs(b1, b2, mode, dtype)
    M, N = b1.shape[0], b2.shape[0]
    # pairs whose circumscribed circles are a pixel apart intersect in nothing: exactly 0 without clipping (what the clipping gives them too)
    r1, r2 = np.hypot(b1[:, 2], b1[:, 3]).astype(F64) / 2, np.hypot(b2[:, 2], b2[:, 3]).astype(F64) / 2
    dist = np.hypot(b1[:, None, 0].astype(F64) - b2[None, :, 0], b1[:, None, 1].astype(F64) - b2[None, :, 1])
    i, j = np.nonzero(dist <= r1[:, None] + r2[None] + 1.0)
    out = np.zeros((M, N), dtype)
    out[i, j] = _rot_pairs(b1[i], b2[j], mode, dtype)
    return out


def nms(boxes, scores, thr, groups=None, rotated=False, dtype=F64, iou=None):
    """greedy NMS -> the kept indices into `boxes`, in descending score order (stable).  `iou`: a precomputed (n, n) matrix instead."""
    scores = np.asarray(scores)
    order = np.argsort(-scores, kind="stable")
    if iou is None:
        iou = box_iou_rotated(boxes, boxes, dtype=dtype) if rotated else bbox_overlaps(boxes, boxes, dtype=dtype)
    groups = np.zeros(len(scores), np.int64) if groups is None else np.asarray(groups)
    dead, keep = np.zeros(len(scores), bool), []
    for i in order:
        if dead[i]:
            continue
        keep.append(int(i))
        dead |= (iou[i] > thr) & (groups == groups[i])
    return np.asarray(keep, np.int64)


KINDS = ("box", "rbox2hbox", "rotated")


def overlaps(gts, priors, kind, dtype=F64):
    """the (K, N) matrix of the three calculators"""
    if kind == "box":
        return bbox_overlaps(gts, priors, dtype=dtype)
    if kind == "rbox2hbox":
        return bbox_overlaps(rbox2hbox(gts, dtype), priors, dtype=dtype)
    return box_iou_rotated(gts, priors, dtype=dtype)


def assign_wrt_overlaps(ov, gt_labels, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True, gt_max_assign_all=True):
    """-> (gt_inds (N) int64, max_overlaps (N), labels (N) int64)"""
    K, N = ov.shape
    gt_inds = np.full(N, -1, np.int64)
    if K == 0 or N == 0:
        if K == 0:
            gt_inds[:] = 0
        return gt_inds, np.zeros(N, ov.dtype), np.full(N, -1, np.int64)
    mx, arg = ov.max(0), ov.argmax(0)
    gmx, garg = ov.max(1), ov.argmax(1)
    lo, hi = neg_iou_thr if isinstance(neg_iou_thr, tuple) else (0.0, neg_iou_thr)
    gt_inds[(mx >= lo) & (mx < hi)] = 0
    pos = mx >= pos_iou_thr
    gt_inds[pos] = arg[pos] + 1
    if match_low_quality:
        for i in range(K):
            if gmx[i] >= min_pos_iou:
                if gt_max_assign_all:
                    gt_inds[ov[i] == gmx[i]] = i + 1
                else:
                    gt_inds[garg[i]] = i + 1
    labels = np.full(N, -1, np.int64)
    labels[gt_inds > 0] = np.asarray(gt_labels, np.int64)[gt_inds[gt_inds > 0] - 1]
    return gt_inds, mx, labels


def assign(gts, priors, gt_labels, kind, dtype=F64, **cfg):
    return assign_wrt_overlaps(overlaps(gts, priors, kind, dtype), gt_labels, **cfg)
