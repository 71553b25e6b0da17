from .feature_fusion_neck import FeatureFusionNeck  # noqa: F401
