from .iou_metric import IoUMetric  # noqa: F401
from .accuracy import Accuracy  # noqa: F401
