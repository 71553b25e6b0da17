"""mmdet's AssignResult: what an assigner hands to a sampler."""


class AssignResult:
    """num_gts; gt_inds (N) int64: -1 ignored, 0 background, i + 1 assigned to gt i; max_overlaps (N); labels (N) int64: the gt's label on positives, else -1"""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels):
        self.num_gts = num_gts
        self.gt_inds = gt_inds
        self.max_overlaps = max_overlaps
        self.labels = labels

    @property
    def num_preds(self):
        return len(self.gt_inds)

    def __repr__(self):
        return "AssignResult(num_gts=%r, gt_inds.shape=%s, max_overlaps.shape=%s, labels.shape=%s)" % (
            self.num_gts, tuple(self.gt_inds.shape), tuple(self.max_overlaps.shape), tuple(self.labels.shape))
