"""The reference's RandomSampler (rotated_detection/random_sampler.py) for the RPN stage, without a host synchronisation: the reference draws
randperm over nonzero(gt_inds > 0) and takes the first num_expected, then the same for gt_inds == 0, and `unique`s both -- three synchronisations and
lists of data-dependent length.  Here every prior draws one uniform key; the num * pos_fraction largest keys among the positives and the
num - n_pos largest among the negatives are that choice in distribution (torch.topk), the counts stay on the device, and the result is the
fixed-size list mtp_amd.ops.rpn_loss reads."""
import torch

from ..registry import TASK_UTILS


class SampleList:
    """inds (num) int64: n_pos positives, then n_neg negatives, indices into the priors the assigner saw; gt_inds (num) int64: on positives the
    assigned gt (0-based); the rest of both rows is padding.  n_pos, n_neg: 0-dim int64 tensors on the device."""

    def __init__(self, inds, gt_inds, n_pos, n_neg):
        self.inds, self.gt_inds, self.n_pos, self.n_neg = inds, gt_inds, n_pos, n_neg

    @property
    def avg_factor(self):
        return self.n_pos + self.n_neg

    @property
    def pos_inds(self):
        """host synchronisation: for inspection and tests"""
        return self.inds[:int(self.n_pos)]

    @property
    def neg_inds(self):
        n = int(self.n_pos)
        return self.inds[n:n + int(self.n_neg)]

    @property
    def pos_assigned_gt_inds(self):
        return self.gt_inds[:int(self.n_pos)]


@TASK_UTILS.register_module(name=["RandomSampler", "MTP_RD_RandomSampler"])
class RandomSampler:
    def __init__(self, num, pos_fraction, neg_pos_ub=-1, add_gt_as_proposals=True, **kwargs):
        if neg_pos_ub >= 0:
            raise NotImplementedError("RandomSampler: neg_pos_ub >= 0 belongs to the RCNN stage, which is not built")
        if add_gt_as_proposals:
            raise NotImplementedError("RandomSampler: add_gt_as_proposals=True belongs to the RCNN stage, which is not built (the RPN configs set False)")
        if kwargs:
            raise TypeError("RandomSampler: unknown arguments %s" % sorted(kwargs))
        if num < 1 or not 0 <= pos_fraction <= 1:
            raise ValueError("RandomSampler: num >= 1 and 0 <= pos_fraction <= 1")
        self.num, self.pos_fraction, self.neg_pos_ub, self.add_gt_as_proposals = int(num), float(pos_fraction), neg_pos_ub, False

    def sample(self, assign_result, pred_instances=None, gt_instances=None, generator=None, pos_inds=None, neg_inds=None, **kwargs):
        """assign_result.gt_inds (N) -> SampleList.  generator: a torch.Generator on gt_inds' device.  pos_inds / neg_inds: an explicit choice (both),
        at most num in all, instead of the draw."""
        gt_inds = assign_result.gt_inds
        dev, N, S = gt_inds.device, gt_inds.shape[0], self.num
        if (pos_inds is None) != (neg_inds is None):
            raise ValueError("RandomSampler.sample: pos_inds and neg_inds come together")
        if pos_inds is not None:
            pos = torch.as_tensor(pos_inds, dtype=torch.int64, device=dev).reshape(-1)
            neg = torch.as_tensor(neg_inds, dtype=torch.int64, device=dev).reshape(-1)
            if pos.numel() + neg.numel() > S:
                raise ValueError("RandomSampler.sample: %d explicit indices for num=%d" % (pos.numel() + neg.numel(), S))
            inds = torch.zeros(S, dtype=torch.int64, device=dev)
            inds[:pos.numel()] = pos
            inds[pos.numel():pos.numel() + neg.numel()] = neg
            n_pos, n_neg = torch.tensor(pos.numel(), device=dev), torch.tensor(neg.numel(), device=dev)
        else:
            cap = int(S * self.pos_fraction)
            keys = torch.rand(N, device=dev, generator=generator)
            is_pos, is_neg = gt_inds > 0, gt_inds == 0
            kp, kn = min(cap, N), min(S, N)
            top_pos = torch.topk(keys.masked_fill(~is_pos, -1.0), kp)[1]
            top_neg = torch.topk(keys.masked_fill(~is_neg, -1.0), kn)[1]
            n_pos = is_pos.sum().clamp(max=kp)
            n_neg = torch.minimum(is_neg.sum(), S - n_pos)
            both = torch.cat([top_pos, top_neg, top_neg.new_zeros(1)])
            j = torch.arange(S, device=dev)
            src = torch.where(j < n_pos, j, kp + j - n_pos)
            inds = both[torch.where(j < n_pos + n_neg, src, torch.full_like(j, kp + kn))]
        slot = torch.arange(S, device=dev)
        gt = torch.where(slot < n_pos, gt_inds[inds.clamp(0, max(N - 1, 0))] - 1, torch.full_like(slot, -1)) if N else torch.full_like(slot, -1)
        return SampleList(inds, gt, n_pos, n_neg)
