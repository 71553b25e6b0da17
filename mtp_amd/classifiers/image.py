"""ImageClassifier (mmpretrain's classifier as every reference scene-classification config composes it: RS_Tasks_Finetune/Scene_Classification/
configs/mtp/*: backbone -> GlobalAveragePooling -> LinearClsHead).  mmpretrain is not part of the reference tree; the class is restated from its
published behaviour with tensors in place of DataSamples (labels (N,) int64).  In a config the backbone type is 'RVSA_MTP_taps' (what mmpretrain
registers as 'RVSA_MTP') or 'InternImage'.
"""
import torch
import torch.nn as nn

from ..registry import MODELS

STAGES = ("backbone", "neck", "pre_logits")


def _cfg(cfg, key, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


@MODELS.register_module()
class ImageClassifier(nn.Module):
    """ImageClassifier(backbone, neck=None, head=None, pretrained=None, train_cfg=None, data_preprocessor=None, init_cfg=None): the three parts are
    modules or config dicts (built through MODELS).  State dict: backbone.*, head.fc.weight, head.fc.bias."""

    def __init__(self, backbone, neck=None, head=None, pretrained=None, train_cfg=None, data_preprocessor=None, init_cfg=None):
        super().__init__()
        if pretrained is not None:
            raise NotImplementedError("ImageClassifier: pretrained=%r is not implemented (load the checkpoint into the backbone)" % (pretrained,))
        if _cfg(train_cfg, "augments"):
            raise NotImplementedError("ImageClassifier: train_cfg.augments %r are not implemented (Mixup / CutMix produce soft labels; the fused "
                                      "loss takes hard labels)" % (_cfg(train_cfg, "augments"),))
        self.backbone = MODELS.build(backbone) if isinstance(backbone, dict) else backbone
        self.neck = MODELS.build(neck) if isinstance(neck, dict) else neck
        self.head = MODELS.build(head) if isinstance(head, dict) else head
        self.train_cfg = train_cfg

    @property
    def with_neck(self):
        return self.neck is not None

    @property
    def with_head(self):
        return self.head is not None

    # ------------------------------------------------------------------ mmpretrain surface
    def extract_feat(self, inputs, stage="neck"):
        """the maps after 'backbone', the vectors after 'neck', or what the head's fc reads ('pre_logits')"""
        if stage not in STAGES:
            raise ValueError('Invalid output stage "%s", please choose from "backbone", "neck" and "pre_logits"' % (stage,))
        x = self.backbone(inputs)
        if stage == "backbone":
            return x
        if self.with_neck:
            x = self.neck(x)
        if stage == "neck":
            return x
        if not self.with_head or not hasattr(self.head, "pre_logits"):
            raise ValueError("No head or the head doesn't implement `pre_logits` method.")
        return self.head.pre_logits(x)

    def loss(self, inputs, labels):
        """-> dict(loss=...)"""
        return self.head.loss(self.extract_feat(inputs), labels)

    @torch.no_grad()
    def predict(self, inputs):
        """eval-mode scores: dict(pred_score (N, K), pred_label (N,))"""
        was_training = self.training
        self.eval()
        try:
            return self.head.predict(self.extract_feat(inputs))
        finally:
            self.train(was_training)

    def forward(self, inputs, labels=None, mode="tensor"):
        if mode == "tensor":
            feats = self.extract_feat(inputs)
            return self.head(feats) if self.with_head else feats
        if mode == "loss":
            return self.loss(inputs, labels)
        if mode == "predict":
            return self.predict(inputs)
        raise RuntimeError('Invalid mode "%s".' % (mode,))
