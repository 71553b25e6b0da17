from .linear_head import LinearClsHead  # noqa: F401
