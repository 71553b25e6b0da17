"""mmcv.ops.RoIAlignRotated under the reference's signature, on the kernels of csrc/roi_head.hip."""
from .roi_align_rotated import RoIAlignRotated, roi_align_rotated  # noqa: F401

__all__ = ["RoIAlignRotated", "roi_align_rotated"]
