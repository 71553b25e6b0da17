"""The RoI head of Oriented R-CNN (mmdet / mmrotate roi_heads), on the kernels of csrc/roi_head.hip and the GEMMs."""
from .bbox_head import Shared2FCBBoxHead  # noqa: F401
from .standard_roi_head import StandardRoIHead  # noqa: F401

MTP_RD_Shared2FCBBoxHead, MTP_RD_StandardRoIHead = Shared2FCBBoxHead, StandardRoIHead
__all__ = ["Shared2FCBBoxHead", "StandardRoIHead", "MTP_RD_Shared2FCBBoxHead", "MTP_RD_StandardRoIHead"]
