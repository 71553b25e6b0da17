from .uper_head import UPerHead  # noqa: F401
from .unet_head import UNetHead  # noqa: F401
