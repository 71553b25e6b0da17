"""MI355X-native DCNv3 core operator (InternImage), mirroring Multi-Task_Pretrain/backbone/ops_dcnv3."""
from .functions import DCNV3_KERNEL, DCNv3Function, dcnv3_backward, dcnv3_forward, dcnv3_kernel  # noqa: F401

__all__ = ["DCNv3Function", "dcnv3_forward", "dcnv3_backward", "dcnv3_kernel", "DCNV3_KERNEL"]
