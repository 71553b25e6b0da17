"""MaxIoUAssigner under the reference's constructor (rotated_detection/max_iou_assigner.py:83-314; mmdet's MaxIoUAssigner for Mask R-CNN).  assign()
runs the fused kernels (mtp_amd.ops.max_iou_assign): no K x N matrix, no loop over the gts on the host."""
import torch

from .. import ops
from ..registry import TASK_UTILS
from .assign_result import AssignResult
from .iou_calculators import box_tensor


def _first(obj, *names):
    for n in names:
        if hasattr(obj, n):
            return getattr(obj, n)
    raise AttributeError("%s has none of %s" % (type(obj).__name__, ", ".join(names)))


@TASK_UTILS.register_module()
class MaxIoUAssigner:
    """mmdet's MaxIoUAssigner: gt_instances.bboxes / .labels (falling back to .rboxes / .rlabels when those are all there is)"""
    GT_BOXES, GT_LABELS, IGNORE_BOXES = ("bboxes", "rboxes"), ("labels", "rlabels"), ("bboxes", "rbboxes")

    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1, ignore_wrt_candidates=True,
                 match_low_quality=True, gpu_assign_thr=-1, iou_calculator=dict(type="BboxOverlaps2D")):
        self.pos_iou_thr = pos_iou_thr
        self.neg_iou_thr = tuple(neg_iou_thr) if isinstance(neg_iou_thr, (tuple, list)) else float(neg_iou_thr)
        if isinstance(self.neg_iou_thr, tuple) and len(self.neg_iou_thr) != 2:
            raise ValueError("MaxIoUAssigner: a neg_iou_thr tuple is (lo, hi)")
        self.min_pos_iou = min_pos_iou
        self.gt_max_assign_all = gt_max_assign_all
        self.ignore_iof_thr = ignore_iof_thr
        self.ignore_wrt_candidates = ignore_wrt_candidates
        self.match_low_quality = match_low_quality
        self.gpu_assign_thr = gpu_assign_thr      # accepted, no effect: there is no matrix to move to the host
        cfg = dict(iou_calculator)
        if isinstance(cfg.get("type"), str):
            for scope in ("mmdet.", "mmrotate."):
                if cfg["type"].startswith(scope):
                    cfg["type"] = cfg["type"][len(scope):]
        self.iou_calculator = TASK_UTILS.build(cfg)

    def assign(self, pred_instances, gt_instances, gt_instances_ignore=None, **kwargs):
        """pred_instances.priors (N, 4 | 5), the gt boxes (K, 4 | 5) and labels (K) of gt_instances under the first of the class's field names that is
        there -- plain tensors or box objects with .tensor -> AssignResult"""
        priors = box_tensor(pred_instances.priors)
        gts = box_tensor(_first(gt_instances, *self.GT_BOXES))
        gt_labels = _first(gt_instances, *self.GT_LABELS)
        if self.ignore_iof_thr > 0 and gt_instances_ignore is not None:
            ign = box_tensor(_first(gt_instances_ignore, *self.IGNORE_BOXES))
            if ign.numel() > 0 and priors.numel() > 0:
                raise NotImplementedError("MaxIoUAssigner: ignore boxes with ignore_iof_thr > 0 are not built (every MTP config sets -1)")
        K, N = gts.shape[0], priors.shape[0]
        if K == 0 or N == 0:
            gt_inds = torch.full((N,), 0 if K == 0 else -1, dtype=torch.int64, device=priors.device)
            return AssignResult(K, gt_inds, torch.zeros(N, dtype=torch.float32, device=priors.device),
                                torch.full((N,), -1, dtype=torch.int64, device=priors.device))
        gts, priors = self.iou_calculator.boxes(gts, priors)
        gt_inds, max_overlaps, labels = ops.max_iou_assign(
            gts.detach().to(torch.float32).contiguous(), priors.detach().to(torch.float32).contiguous(), gt_labels.to(torch.int64).contiguous(),
            self.iou_calculator.kind, self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou, self.match_low_quality, self.gt_max_assign_all)
        return AssignResult(K, gt_inds, max_overlaps, labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels):
        """the reference's steps on a (K, N) matrix the caller already holds, in torch: not a hot path"""
        K, N = overlaps.shape
        gt_inds = overlaps.new_full((N,), -1, dtype=torch.long)
        if K == 0 or N == 0:
            if K == 0:
                gt_inds[:] = 0
            return AssignResult(K, gt_inds, overlaps.new_zeros((N,)), overlaps.new_full((N,), -1, dtype=torch.long))
        max_overlaps, argmax = overlaps.max(dim=0)
        gt_max, gt_argmax = overlaps.max(dim=1)
        lo, hi = self.neg_iou_thr if isinstance(self.neg_iou_thr, tuple) else (0, self.neg_iou_thr)
        gt_inds[(max_overlaps >= lo) & (max_overlaps < hi)] = 0
        pos = max_overlaps >= self.pos_iou_thr
        gt_inds[pos] = argmax[pos] + 1
        if self.match_low_quality:
            for i in range(K):
                if gt_max[i] >= self.min_pos_iou:
                    if self.gt_max_assign_all:
                        gt_inds[overlaps[i, :] == gt_max[i]] = i + 1
                    else:
                        gt_inds[gt_argmax[i]] = i + 1
        labels = gt_inds.new_full((N,), -1)
        pos = gt_inds > 0
        labels[pos] = gt_labels.to(torch.long)[gt_inds[pos] - 1]
        return AssignResult(K, gt_inds, max_overlaps, labels)


@TASK_UTILS.register_module()
class MTP_RD_MaxIoUAssigner(MaxIoUAssigner):
    """the reference's rotated-detection assigner (rotated_detection/max_iou_assigner.py:190-194): it reads gt_instances.rboxes / .rlabels (ignore boxes:
    .rbboxes), so those come first here -- a gt_instances that carries horizontal and rotated fields side by side feeds the rotated ones; .bboxes /
    .labels are the fallback"""
    GT_BOXES, GT_LABELS, IGNORE_BOXES = ("rboxes", "bboxes"), ("rlabels", "labels"), ("rbboxes", "bboxes")
