from .iou_metric import IoUMetric  # noqa: F401
from .accuracy import Accuracy  # noqa: F401
from .dota_metric import DOTAMetric, eval_rbbox_map, rbox2qbox  # noqa: F401
from .coco_metric import CocoMetric, eval_coco  # noqa: F401
