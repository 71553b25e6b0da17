"""RoI extractors of the detection heads (mmdet, mmrotate), on the kernels of csrc/roi_head.hip and csrc/mask_head.hip."""
from .rotated_single_level import RotatedSingleRoIExtractor  # noqa: F401
from .single_level import SingleRoIExtractor  # noqa: F401

__all__ = ["RotatedSingleRoIExtractor", "SingleRoIExtractor"]
