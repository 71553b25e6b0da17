"""LinearClsHead (mmpretrain's linear classification head with CrossEntropyLoss, as every reference scene-classification config sets it:
`head=dict(type='LinearClsHead', num_classes=10 | 45, in_channels=768 | 1024 | 1536, loss=dict(type='CrossEntropyLoss', loss_weight=1.0),
topk=(1, 5))`) on the kernels of csrc/cls_head.hip.

mmpretrain is not part of the reference tree, so this restates the class from its published behaviour: `fc = nn.Linear(in_channels, num_classes)`
initialised N(0, 0.01) / 0 on the last of the neck's vectors, softmax cross-entropy averaged over the batch, `predict` = softmax scores and their
arg-max.  The linear layer, the softmax, the loss and dlogits are ONE launch (mtp_cls_ce), the three gradients another (mtp_cls_head_bwd).  Two
surfaces over the same kernels: autograd (`forward`, `loss`), and `loss_and_grads` in DataParallelTrainer.step's form, which pools the backbone's
last map itself and uses no autograd.
"""
import torch
import torch.nn as nn

from .. import ops
from ..registry import MODELS

F32 = torch.float32


class _LinearFn(torch.autograd.Function):
    """pooled (N, C), w, b -> logits (N, K)"""

    @staticmethod
    def forward(ctx, pooled, w, b):
        pooled, w, b = pooled.contiguous(), w.contiguous(), b.contiguous()
        ctx.save_for_backward(pooled, w)
        return ops.cls_ce(pooled, w, b, outputs=("logits",))["logits"]

    @staticmethod
    def backward(ctx, g):
        pooled, w = ctx.saved_tensors
        dw, db, dp = torch.empty_like(w), torch.empty(w.shape[0], device=w.device, dtype=F32), torch.empty_like(pooled)
        ops.cls_head_bwd(g.contiguous(), pooled, w, dw, db, dp)
        return dp, dw, db


class _LossFn(torch.autograd.Function):
    """pooled (N, C), w, b, labels -> loss (); the backward is the same mtp_cls_head_bwd launch loss_and_grads makes"""

    @staticmethod
    def forward(ctx, pooled, w, b, labels, loss_weight):
        pooled, w, b = pooled.contiguous(), w.contiguous(), b.contiguous()
        out = ops.cls_ce(pooled, w, b, labels, loss_weight)
        ctx.save_for_backward(pooled, w, out["dlogits"])
        return out["loss"]

    @staticmethod
    def backward(ctx, dloss):
        pooled, w, dl = ctx.saved_tensors
        dw, db, dp = torch.empty_like(w), torch.empty(w.shape[0], device=w.device, dtype=F32), torch.empty_like(pooled)
        ops.cls_head_bwd(dl, pooled, w, dw, db, dp)
        return dp * dloss, dw * dloss, db * dloss, None, None


@MODELS.register_module()
class LinearClsHead(nn.Module):
    """LinearClsHead(num_classes, in_channels, loss=dict(type='CrossEntropyLoss', loss_weight=1.0), topk=(1,), cal_acc=False, init_cfg=None)"""

    def __init__(self, num_classes, in_channels, loss=dict(type="CrossEntropyLoss", loss_weight=1.0), topk=(1,), cal_acc=False, init_cfg=None):
        super().__init__()
        lt = str(loss.get("type", "CrossEntropyLoss")) if isinstance(loss, dict) else None
        if lt is not None and lt.startswith("mmpretrain."):
            lt = lt[len("mmpretrain."):]      # the scoped name of the same loss
        if lt != "CrossEntropyLoss" or loss.get("use_sigmoid", False) or loss.get("use_soft", False) or loss.get("class_weight") is not None \
                or loss.get("pos_weight") is not None or loss.get("reduction", "mean") != "mean":
            raise NotImplementedError("LinearClsHead: loss %r is not implemented (CrossEntropyLoss, softmax, reduction='mean', no class / positive "
                                      "weights, hard labels)" % (loss,))
        if cal_acc:
            raise NotImplementedError("LinearClsHead: cal_acc=True is not implemented (cal_acc=%r; use mtp_amd.Accuracy on predict()'s scores)" % (cal_acc,))
        if init_cfg is not None:
            raise NotImplementedError("LinearClsHead: init_cfg %r is not implemented (None: fc ~ N(0, 0.01), bias 0)" % (init_cfg,))
        if int(num_classes) <= 0:
            raise ValueError("num_classes=%s must be a positive integer" % (num_classes,))
        self.num_classes, self.in_channels = int(num_classes), int(in_channels)
        self.topk = (int(topk),) if isinstance(topk, int) else tuple(int(k) for k in topk)
        if any(k > self.num_classes or k < 1 for k in self.topk):
            raise ValueError("LinearClsHead: topk %s outside [1, num_classes = %d]" % (self.topk, self.num_classes))
        self.cal_acc, self.loss_weight = False, float(loss.get("loss_weight", 1.0))
        self.fc = nn.Linear(self.in_channels, self.num_classes)
        nn.init.normal_(self.fc.weight, 0.0, 0.01)
        nn.init.constant_(self.fc.bias, 0.0)

    def trained_parameter_names(self):
        """the parameters a training step updates"""
        return [n for n, p in self.named_parameters() if p.requires_grad]

    # ------------------------------------------------------------------ mmpretrain surface
    def pre_logits(self, feats):
        """the last of the neck's outputs: the head has no layers in front of fc"""
        return feats[-1] if isinstance(feats, (tuple, list)) else feats

    def _vector(self, feats):
        x = self.pre_logits(feats)
        if x.dim() != 2 or x.shape[1] != self.in_channels or x.dtype != F32:
            raise ValueError("LinearClsHead: expected the neck's (N, %d) f32 vectors, got %s %s" % (self.in_channels, tuple(x.shape), x.dtype))
        return x

    def forward(self, feats):
        """-> logits (N, num_classes) f32"""
        return _LinearFn.apply(self._vector(feats), self.fc.weight, self.fc.bias)

    def loss(self, feats, labels):
        """labels (N,) int64 instead of DataSamples -> dict(loss=...)"""
        return dict(loss=_LossFn.apply(self._vector(feats), self.fc.weight, self.fc.bias, labels.contiguous(), self.loss_weight))

    @torch.no_grad()
    def predict(self, feats):
        """-> dict(pred_score (N, num_classes) softmax, pred_label (N,) int64)"""
        out = ops.cls_ce(self._vector(feats).contiguous(), self.fc.weight.contiguous(), self.fc.bias.contiguous())
        return dict(pred_score=out["prob"], pred_label=out["pred"])

    # ------------------------------------------------------------------ fast path
    def loss_and_grads(self, labels):
        """fn(feats) -> (loss, dfeats) for DataParallelTrainer.step: feats are the backbone's NCHW maps, the head pools the last one itself; its own
        parameter gradients are accumulated into .grad; dfeats is None for every map but the last, whose gradient has the map's dtype.  Four launches,
        no autograd and no host synchronisation inside fn (the labels' range is checked here, once)."""
        labels = labels.contiguous()
        ops._check_labels("LinearClsHead", labels, labels.shape[0], self.num_classes)

        def fn(feats):
            x = feats[-1]
            if x.dim() != 4 or x.shape[1] != self.in_channels or x.shape[0] != labels.shape[0]:
                raise ValueError("LinearClsHead: expected a last map of shape (%d, %d, H, W), got %s" % (labels.shape[0], self.in_channels, tuple(x.shape)))
            w, b = self.fc.weight.detach(), self.fc.bias.detach()
            pooled = ops.gap_fwd(x.detach().contiguous())
            out = ops.cls_ce(pooled, w, b, labels, self.loss_weight, check_labels=False)
            acc = self.fc.weight.grad is not None and self.fc.bias.grad is not None
            if not acc:
                self.fc.weight.grad, self.fc.bias.grad = torch.empty_like(w), torch.empty_like(b)
            dp = ops._scratch(tuple(pooled.shape), pooled.device, F32)
            ops.cls_head_bwd(out["dlogits"], pooled, w, self.fc.weight.grad, self.fc.bias.grad, dp, accumulate=acc)
            dx = ops.gap_bwd(dp, ops._scratch(tuple(x.shape), x.device, x.dtype))
            return out["loss"], [None] * (len(feats) - 1) + [dx]
        return fn
