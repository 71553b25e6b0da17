from .iou_metric import IoUMetric  # noqa: F401
