"""IoUMetric (mmseg IoUMetric as the reference uses it: Multi-Task_Pretrain/semantic_segmentation/metric.py, MTP_SS_Metric) on the kernels of
csrc/seg_eval.hip.

The reference keeps four float histograms per image on the host (three masked torch.histc calls and a .cpu() each).  Here the three independent ones
-- intersect, prediction, label -- are int64 counters that stay on the device: `process` adds an existing prediction's, `process_logits` takes the
arg-max of a logit accumulator and counts in the same launch.  `compute_metrics` makes the one host sync, derives union = pred + label - intersect and
evaluates the reference's formulas in float64.
"""
import warnings
from collections import OrderedDict

import numpy as np
import torch

from .. import ops

ALLOWED_METRICS = ("mIoU", "mDice", "mFscore")


class IoUMetric:
    """IoUMetric(num_classes, ignore_index=255, iou_metrics=['mIoU'], nan_to_num=None, beta=1).  `areas`: (3, num_classes) int64 = (intersect, pred,
    label), None until the first batch.  `reduce`: None, or a callable summing an int64 tensor over the ranks (a test hook; with torch.distributed up
    and more than one rank the counters go through all_reduce)."""

    def __init__(self, num_classes, ignore_index=255, iou_metrics=("mIoU",), nan_to_num=None, beta=1, **kwargs):
        if isinstance(iou_metrics, str):
            iou_metrics = [iou_metrics]
        if not set(iou_metrics).issubset(ALLOWED_METRICS):
            raise KeyError("metrics %s is not supported" % (list(iou_metrics),))
        if not 0 < int(num_classes) <= ops.SEG_MAX_CLASSES:
            raise ValueError("IoUMetric: num_classes must be in [1, %d] (got %s)" % (ops.SEG_MAX_CLASSES, num_classes))
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self.metrics, self.nan_to_num, self.beta = list(iou_metrics), nan_to_num, beta
        self.areas = None
        self.reduce = None
        self.per_class = None        # after compute_metrics: the per-class arrays (IoU, Acc, Dice, Fscore, Precision, Recall), fractions

    # ------------------------------------------------------------------ accumulation
    def reset(self):
        self.areas = None
        self.per_class = None

    def _counters(self, device):
        if self.areas is None:
            self.areas = torch.zeros(3, self.num_classes, device=device, dtype=torch.int64)
        return self.areas

    @staticmethod
    def _labels(labels):
        if labels.dim() == 4:
            labels = labels.squeeze(1)
        return labels.contiguous()

    def process(self, pred, labels):
        """pred, labels: (N, H, W) or (H, W), uint8 / int64, on the device"""
        labels = self._labels(labels)
        pred = pred.contiguous().view(labels.shape)
        ops.seg_areas(pred, labels, self.num_classes, self._counters(pred.device), self.ignore_index)

    def process_logits(self, acc, labels, cy=None, cx=None, pred=None, seg_logits=None):
        """acc (N, H, W, >= num_classes) f32 channels-last logits (a window sum with its counts cy / cx, or plain logits): the arg-max and the
        areas in one launch; pred / seg_logits as in ops.seg_argmax_areas"""
        return ops.seg_argmax_areas(acc, self.num_classes, cy, cx, pred, seg_logits, self._labels(labels), self._counters(acc.device), self.ignore_index)

    # ------------------------------------------------------------------ evaluation
    def _reduce_fn(self):
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            def red(t):
                torch.distributed.all_reduce(t)
                return t
            return red
        return self.reduce

    def total_areas(self):
        """(intersect, union, pred, label) int64 on the host, summed over the ranks: the one synchronisation"""
        if self.areas is None:
            raise RuntimeError("IoUMetric: nothing processed yet")
        a = self.areas.clone()
        red = self._reduce_fn()
        if red is not None:
            a = red(a)
        a = a.cpu()
        return a[0], a[1] + a[2] - a[0], a[1], a[2]

    def compute_metrics(self):
        ret = self.total_area_to_metrics(*self.total_areas(), self.metrics, self.nan_to_num, self.beta)
        out = OrderedDict()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)      # nanmean of an all-NaN column
            for k, v in ret.items():
                out[k if k == "aAcc" else "m" + k] = np.round(np.nanmean(v) * 100, 2)
        ret.pop("aAcc", None)
        self.per_class = ret
        return dict(out)

    @staticmethod
    def total_area_to_metrics(total_area_intersect, total_area_union, total_area_pred_label, total_area_label, metrics=("mIoU",), nan_to_num=None, beta=1):
        """the reference's formulas (metric.py:203-286) in float64 -> OrderedDict of numpy arrays (aAcc a scalar); 0 / 0 = NaN as there"""
        if isinstance(metrics, str):
            metrics = [metrics]
        if not set(metrics).issubset(ALLOWED_METRICS):
            raise KeyError("metrics %s is not supported" % (list(metrics),))
        I, U, P, L = (t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)
                      for t in (total_area_intersect, total_area_union, total_area_pred_label, total_area_label))
        with np.errstate(divide="ignore", invalid="ignore"):
            ret = OrderedDict(aAcc=I.sum() / L.sum())
            for m in metrics:
                if m == "mIoU":
                    ret["IoU"], ret["Acc"] = I / U, I / L
                elif m == "mDice":
                    ret["Dice"], ret["Acc"] = 2 * I / (P + L), I / L
                else:
                    precision, recall = I / P, I / L
                    ret["Fscore"] = (1 + beta ** 2) * (precision * recall) / ((beta ** 2 * precision) + recall)
                    ret["Precision"], ret["Recall"] = precision, recall
        ret = OrderedDict((k, np.asarray(v)) for k, v in ret.items())
        if nan_to_num is not None:
            ret = OrderedDict((k, np.nan_to_num(v, nan=nan_to_num)) for k, v in ret.items())
        return ret
