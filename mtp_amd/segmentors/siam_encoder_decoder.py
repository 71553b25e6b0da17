"""SiamEncoderDecoder (open-cd's siamese segmentor: every reference change-detection config's `model=dict(type='SiamEncoderDecoder', backbone=...,
neck=dict(type='FeatureFusionNeck', ...), decode_head=dict(type='UNetHead', ...), test_cfg=dict(mode='whole'))`).

open-cd is not part of the reference tree; this restates the class from open-cd's published behaviour: the (N, 2 * backbone_inchannels, H, W) input
(the DualInputSegDataPreProcessor's output: the "from" image's channels, then the "to" image's) is split, the ONE backbone runs on both images
(shared weights) and the neck fuses the two feature tuples.  Here the backbone runs once on the 2N-batch cat([img_from, img_to]), which is the same
computation (BatchNorm-free backbones; drop-path masks are drawn per sample either way).  Inference, padding / ori_shape handling and the IoUMetric
path are EncoderDecoder's.
"""
import torch

from ..registry import MODELS
from .encoder_decoder import EncoderDecoder


@MODELS.register_module()
class SiamEncoderDecoder(EncoderDecoder):
    def __init__(self, backbone, decode_head, neck=None, test_cfg=None, backbone_inchannels=3, auxiliary_head=None, train_cfg=None,
                 data_preprocessor=None, pretrained=None, init_cfg=None):
        super().__init__(backbone, decode_head, test_cfg=test_cfg, auxiliary_head=auxiliary_head, train_cfg=train_cfg,
                         data_preprocessor=data_preprocessor, pretrained=pretrained, init_cfg=init_cfg)
        if neck is None:
            raise ValueError("SiamEncoderDecoder needs a neck that fuses the two images' features (FeatureFusionNeck)")
        self.neck = MODELS.build(neck) if isinstance(neck, dict) else neck
        self.backbone_inchannels = int(backbone_inchannels)

    def split(self, inputs):
        """(N, 2c, H, W) -> the 2N-batch (2N, c, H, W): 'from' images first, 'to' images last"""
        c = self.backbone_inchannels
        if inputs.dim() != 4 or inputs.shape[1] != 2 * c:
            raise ValueError("SiamEncoderDecoder: expected (N, %d, H, W) inputs, got %s" % (2 * c, tuple(inputs.shape)))
        return torch.cat([inputs[:, :c], inputs[:, c:]], 0)

    def extract_feat(self, inputs):
        feats = self.backbone(self.split(inputs))
        if hasattr(self.neck, "forward_batch"):        # FeatureFusionNeck reads both halves out of the 2N-batch maps in place
            return self.neck.forward_batch(feats)
        N = inputs.shape[0]
        return self.neck([f[:N] for f in feats], [f[N:] for f in feats])
