from .feature_fusion_neck import FeatureFusionNeck  # noqa: F401
from .global_average_pooling import GlobalAveragePooling  # noqa: F401
