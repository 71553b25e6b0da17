"""mmcv.ops.RoIAlignRotated and mmcv.ops.RoIAlign under the reference's signatures, on the kernels of csrc/roi_head.hip and csrc/mask_head.hip."""
from .roi_align import RoIAlign, roi_align  # noqa: F401
from .roi_align_rotated import RoIAlignRotated, roi_align_rotated  # noqa: F401

__all__ = ["RoIAlign", "RoIAlignRotated", "roi_align", "roi_align_rotated"]
