"""Accuracy (mmpretrain's top-k accuracy, `val_evaluator = dict(type='Accuracy', topk=(1, 5))` in every reference scene-classification config) on
mtp_cls_hits (csrc/cls_head.hip), shaped like IoUMetric: int64 counters that stay on the device, one launch per batch, one host synchronisation in
compute_metrics.

mmpretrain takes the top max(topk) labels by score and counts a sample for k when its label is among the first k and that score exceeds `thrs`.  The
kernel needs no sort: the label's position is the number of classes that score higher plus the equal-scoring classes in front of it.
"""
from collections import OrderedDict

import torch

from .. import ops
from ..registry import MODELS


@MODELS.register_module()
class Accuracy:
    """Accuracy(topk=(1,), thrs=0.0).  `counters`: (len(topk) + 1,) int64 = hits per k, then the number of samples; None until the first batch.
    `reduce`: None, or a callable summing an int64 tensor over the ranks (a test hook; with torch.distributed up and more than one rank the counters go
    through all_reduce).  thrs: a float, or None for no threshold."""

    def __init__(self, topk=(1,), thrs=0.0, **kwargs):
        self.topk = (int(topk),) if isinstance(topk, int) else tuple(int(k) for k in topk)
        if not self.topk or len(self.topk) > ops.CLS_MAX_TOPK or any(k < 1 for k in self.topk) or list(self.topk) != sorted(set(self.topk)):
            raise ValueError("Accuracy: topk must be 1 to %d ascending positive ints (got %s)" % (ops.CLS_MAX_TOPK, self.topk))
        if isinstance(thrs, (tuple, list)):
            if len(thrs) != 1:
                raise NotImplementedError("Accuracy: several thresholds %r are not implemented (no MTP config sets one)" % (thrs,))
            thrs = thrs[0]
        self.thrs = None if thrs is None else float(thrs)
        self.counters = None
        self.reduce = None

    def reset(self):
        self.counters = None

    def process(self, scores, labels):
        """scores (N, K) f32 on the device, labels (N,) int64: one launch"""
        if scores.dim() != 2:
            raise ValueError("Accuracy: scores must be (N, K), got %s" % (tuple(scores.shape),))
        if self.topk[-1] > scores.shape[1]:
            raise ValueError("Accuracy: topk %s exceeds the %d classes" % (self.topk, scores.shape[1]))
        if self.counters is None:
            self.counters = torch.zeros(len(self.topk) + 1, device=scores.device, dtype=torch.int64)
        ops.cls_hits(scores.contiguous(), labels.contiguous().view(-1), self.topk, self.counters, self.thrs)

    def _reduce_fn(self):
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            def red(t):
                torch.distributed.all_reduce(t)
                return t
            return red
        return self.reduce

    def totals(self):
        """(hits per k ..., samples) as Python ints, summed over the ranks: the one synchronisation"""
        if self.counters is None:
            raise RuntimeError("Accuracy: nothing processed yet")
        c = self.counters.clone()
        red = self._reduce_fn()
        if red is not None:
            c = red(c)
        return [int(v) for v in c.cpu().tolist()]

    def compute_metrics(self):
        """-> OrderedDict('accuracy/top1': ..., 'accuracy/top5': ...) in percent, float64"""
        return self.counts_to_metrics(self.totals(), self.topk)

    @staticmethod
    def counts_to_metrics(counts, topk):
        *hits, total = [int(v) for v in counts]
        if len(hits) != len(topk):
            raise ValueError("Accuracy: %d counters for topk %s" % (len(hits), tuple(topk)))
        return OrderedDict(("accuracy/top%d" % k, (float(h) * 100.0 / float(total)) if total else float("nan")) for k, h in zip(topk, hits))
