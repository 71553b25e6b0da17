from .uper_head import UPerHead  # noqa: F401
