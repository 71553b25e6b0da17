"""Dense detection heads on libmtp_hip.so: the oriented RPN of Oriented R-CNN (csrc/rpn.hip)."""
from .oriented_rpn_head import MTP_RD_OrientedRPNHead, OrientedRPNHead  # noqa: F401

__all__ = ["OrientedRPNHead", "MTP_RD_OrientedRPNHead"]
