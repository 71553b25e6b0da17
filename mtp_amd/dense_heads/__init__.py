"""Dense detection heads on libmtp_hip.so: the oriented RPN of Oriented R-CNN (csrc/rpn.hip) and the horizontal RPN of Mask R-CNN
(csrc/hbox_head.hip)."""
from .oriented_rpn_head import MTP_RD_OrientedRPNHead, OrientedRPNHead  # noqa: F401
from .rpn_head import MTP_IS_RPNHead, RPNHead  # noqa: F401

__all__ = ["OrientedRPNHead", "MTP_RD_OrientedRPNHead", "RPNHead", "MTP_IS_RPNHead"]
