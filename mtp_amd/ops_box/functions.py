"""bbox_overlaps (mmdet.structures.bbox), box_iou_rotated, nms, nms_rotated, batched_nms (mmcv.ops) with the reference's signatures, on the kernels of
csrc/box_ops.hip.  The reference calls them at instance_segmentation/rpn_head.py:284, rotated_detection/rpn_head.py:284, dense_head.py:513,591 and
through the test_cfg dicts of mask_rcnn.py / oriented_rcnn.py.  Sorting is torch.sort(descending=True, stable=True) on the device: among equal scores
the lower input index comes first (mmcv leaves that open).  Empty inputs return empty results on any device without touching the library."""
import torch

from .. import ops


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def bbox_overlaps(bboxes1, bboxes2, mode="iou", is_aligned=False, eps=1e-6):
    """(M, 4) x (N, 4) boxes x1, y1, x2, y2 -> (M, N) overlaps, or (M,) when is_aligned.  No +1; union = max(a1 + a2 - inter, eps); 'iof' divides by
    max(a1, eps)."""
    if mode == "giou":
        raise NotImplementedError("bbox_overlaps: mode 'giou' is not built (no MTP config asks for it)")
    if mode not in ("iou", "iof"):
        raise ValueError("bbox_overlaps: mode must be 'iou' or 'iof', got %r" % (mode,))
    if bboxes1.dim() != 2 or bboxes2.dim() != 2:
        raise NotImplementedError("bbox_overlaps: batch dimensions are not built; pass (M, 4) and (N, 4)")
    if bboxes1.shape[1] != 4 or bboxes2.shape[1] != 4:
        raise ValueError("bbox_overlaps: boxes must have 4 columns")
    M, N = bboxes1.shape[0], bboxes2.shape[0]
    if is_aligned and M != N:
        raise ValueError("bbox_overlaps: is_aligned needs as many bboxes1 as bboxes2")
    if M * N == 0:
        return bboxes1.new_zeros((M,) if is_aligned else (M, N), dtype=torch.float32)
    return ops.box_iou(_f32(bboxes1), _f32(bboxes2), iof=mode == "iof", aligned=is_aligned, eps=eps)


def box_iou_rotated(bboxes1, bboxes2, mode="iou", aligned=False, clockwise=True):
    """(M, 5) x (N, 5) boxes cx, cy, w, h, theta (radians) -> (M, N), or (M,) when aligned; 0 when either area is below 1e-14.  `clockwise` is accepted
    and has no effect: the intersection area does not depend on the angle's sign convention as long as both boxes share it."""
    if mode not in ("iou", "iof"):
        raise ValueError("box_iou_rotated: mode must be 'iou' or 'iof', got %r" % (mode,))
    if bboxes1.dim() != 2 or bboxes2.dim() != 2 or bboxes1.shape[1] != 5 or bboxes2.shape[1] != 5:
        raise ValueError("box_iou_rotated: boxes must be (M, 5) and (N, 5)")
    M, N = bboxes1.shape[0], bboxes2.shape[0]
    if aligned and M != N:
        raise ValueError("box_iou_rotated: aligned needs as many bboxes1 as bboxes2")
    if M * N == 0:
        return bboxes1.new_zeros((M,) if aligned else (M, N), dtype=torch.float32)
    return ops.box_iou(_f32(bboxes1), _f32(bboxes2), rotated=True, iof=mode == "iof", aligned=aligned)


def _keep(boxes, scores, iou_threshold, groups, rotated, max_num):
    """-> indices into boxes of the kept ones, in descending score order; one host synchronisation, for the count"""
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=boxes.device)
    ops.check_nms_count(n)      # before the sort
    order = torch.sort(scores.detach(), descending=True, stable=True)[1]
    g = None if groups is None else groups.detach().to(torch.int64)[order].contiguous()
    keep, count = ops.nms_sorted(_f32(boxes)[order].contiguous(), iou_threshold, g, rotated, max_num)
    return order[keep[:int(count.item())]]


def nms(boxes, scores, iou_threshold, offset=0, score_threshold=0, max_num=-1):
    """boxes (n, 4), scores (n) -> (dets (k, 5) = boxes and scores of the kept, inds (k) into the caller's input, descending score).  Suppression is
    `iou > iou_threshold`.  score_threshold > 0 drops the boxes with score <= score_threshold first; max_num > 0 keeps the first max_num."""
    if offset != 0:
        raise NotImplementedError("nms: offset=1 (the legacy +1 pixel convention) is not built; every MTP config runs offset=0")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or scores.shape != boxes.shape[:1]:
        raise ValueError("nms: boxes must be (n, 4) and scores (n,)")
    src = None
    if score_threshold > 0:
        src = torch.nonzero(scores > score_threshold).squeeze(1)
        boxes, scores = boxes[src], scores[src]
    inds = _keep(boxes, scores, iou_threshold, None, False, max_num)
    dets = torch.cat([boxes[inds], scores[inds].reshape(-1, 1).to(boxes.dtype)], 1)
    return dets, (inds if src is None else src[inds])


def nms_rotated(dets, scores, iou_threshold, labels=None, clockwise=True):
    """dets (n, 5) cx, cy, w, h, theta, scores (n), labels (n) or None: boxes of different labels do not suppress each other
    -> (dets (k, 6), inds (k)), descending score"""
    if dets.dim() != 2 or dets.shape[1] != 5 or scores.shape != dets.shape[:1]:
        raise ValueError("nms_rotated: dets must be (n, 5) and scores (n,)")
    inds = _keep(dets, scores, iou_threshold, labels, True, -1)
    return torch.cat([dets[inds], scores[inds].reshape(-1, 1).to(dets.dtype)], 1), inds


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """NMS within each value of idxs (all together when class_agnostic).  nms_cfg: type 'nms' (boxes (n, 4)) or 'nms_rotated' (boxes (n, 5)),
    iou_threshold, optionally max_num; split_thr is accepted and ignored -- the ids go to the kernel as group ids, so there is neither a coordinate offset
    nor a per-class loop to choose between.  nms_cfg None: no suppression.  -> (dets (k, 5 | 6), keep (k)), descending score"""
    if nms_cfg is None:
        keep = torch.sort(scores, descending=True, stable=True)[1]
        return torch.cat([boxes[keep], scores[keep].reshape(-1, 1)], 1), keep
    cfg = dict(nms_cfg)
    kind = cfg.pop("type", "nms")
    if kind not in ("nms", "nms_rotated"):
        raise NotImplementedError("batched_nms: type %r is not built ('nms' and 'nms_rotated' are)" % (kind,))
    cfg.pop("split_thr", None)
    class_agnostic = cfg.pop("class_agnostic", class_agnostic)
    max_num = cfg.pop("max_num", -1)
    thr = cfg.pop("iou_threshold")
    if kind == "nms" and cfg.pop("offset", 0) != 0:
        raise NotImplementedError("batched_nms: offset=1 is not built")
    if cfg:
        raise TypeError("batched_nms: unknown nms_cfg keys %s" % sorted(cfg))
    cols = 5 if kind == "nms_rotated" else 4
    if boxes.dim() != 2 or boxes.shape[1] != cols or scores.shape != boxes.shape[:1] or idxs.shape != scores.shape:
        raise ValueError("batched_nms: type %r takes boxes (n, %d), scores (n,) and idxs (n,)" % (kind, cols))
    keep = _keep(boxes, scores, thr, None if class_agnostic else idxs, kind == "nms_rotated", max_num)
    return torch.cat([boxes[keep], scores[keep].reshape(-1, 1).to(boxes.dtype)], 1), keep
