"""The RoI heads (mmdet / mmrotate roi_heads): the box head of Oriented R-CNN on the kernels of csrc/roi_head.hip, the mask branch of Mask R-CNN on
those of csrc/mask_head.hip, the box half of Mask R-CNN on those of csrc/hbox_head.hip, all over the GEMMs."""
from .bbox_head import Shared2FCBBoxHead  # noqa: F401
from .hbox_head import HBoxShared2FCBBoxHead  # noqa: F401
from .hbox_roi_head import HBoxRoIHead  # noqa: F401
from .mask_head import FCNMaskHead  # noqa: F401
from .mask_roi_head import MaskRoIHead  # noqa: F401
from .standard_roi_head import StandardRoIHead  # noqa: F401

MTP_RD_Shared2FCBBoxHead, MTP_RD_StandardRoIHead = Shared2FCBBoxHead, StandardRoIHead
MTP_IS_FCNMaskHead, MTP_IS_StandardRoIHead = FCNMaskHead, MaskRoIHead
MTP_IS_Shared2FCBBoxHead, MTP_IS_BBoxRoIHead = HBoxShared2FCBBoxHead, HBoxRoIHead
__all__ = ["Shared2FCBBoxHead", "StandardRoIHead", "MTP_RD_Shared2FCBBoxHead", "MTP_RD_StandardRoIHead", "FCNMaskHead", "MaskRoIHead", "MTP_IS_FCNMaskHead",
           "MTP_IS_StandardRoIHead", "HBoxShared2FCBBoxHead", "HBoxRoIHead", "MTP_IS_Shared2FCBBoxHead", "MTP_IS_BBoxRoIHead"]
