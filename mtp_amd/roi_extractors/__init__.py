"""RoI extractors of the detection heads (mmrotate), on the kernels of csrc/roi_head.hip."""
from .rotated_single_level import RotatedSingleRoIExtractor  # noqa: F401

__all__ = ["RotatedSingleRoIExtractor"]
