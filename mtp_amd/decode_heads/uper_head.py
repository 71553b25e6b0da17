"""UPerHead (mmseg 1.x UPerHead / BaseDecodeHead surface, as the reference uses it: RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/
uper_head.py, the semantic-segmentation configs, Multi-Task_Pretrain/models.py:112-143) on the HIP schedule of engine_uper, under BaseDecodeHead.

State-dict keys and shapes are mmcv / mmseg's (ConvModule = conv without bias -> bn -> ReLU), so an mmseg checkpoint loads strictly.  The forward
runs through BaseDecodeHead's torch.autograd.Function over the engine, so the head trains under plain autograd; `loss_and_grads` is the fast path
that runs forward, loss and backward without autograd.
"""
import torch
import torch.nn as nn

from ..engine_uper import UperEngine
from ..registry import MODELS
from .base import CLS, F32, BaseDecodeHead, _rows


class _ConvModule(nn.Module):
    """mmcv ConvModule(conv -> bn -> ReLU), bias='auto' = no conv bias under a norm; init as mmcv (kaiming fan_out relu, BN 1 / 0)"""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.bn.weight, 1.0)
        nn.init.constant_(self.bn.bias, 0.0)


@MODELS.register_module()
class UPerHead(BaseDecodeHead):
    """mmseg UPerHead(pool_scales, in_channels, channels, num_classes, in_index, dropout_ratio, norm_cfg, act_cfg, align_corners, ignore_index,
    loss_decode).  precision: 'fp32' (f32 GEMM operands) or 'bf16'.  slice_classes: the MTP pretraining arrangement (Multi-Task_Pretrain/models.py:
    129-143) -- one Dropout2d(0.1) + Conv2d(channels, classes_i, 1) classifier per dataset slice (semseghead_{1,2,3}), used by loss_and_grads(slices=3)."""

    engine = UperEngine

    def __init__(self, in_channels, channels, num_classes, pool_scales=(1, 2, 3, 6), in_index=(0, 1, 2, 3), dropout_ratio=0.1,
                 norm_cfg=dict(type="BN", requires_grad=True), act_cfg=dict(type="ReLU"), align_corners=False, ignore_index=255,
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), conv_cfg=None, input_transform="multiple_select",
                 precision="fp32", slice_classes=None, init_cfg=None, **kwargs):
        super().__init__(num_classes, in_index, dropout_ratio, norm_cfg, act_cfg, align_corners, ignore_index, loss_decode, conv_cfg, input_transform,
                         precision, **kwargs)
        in_channels = list(in_channels)
        if channels % 8 or any(c % 8 for c in in_channels):
            raise NotImplementedError("UPerHead: channels and in_channels must be multiples of 8 (the GEMMs' operand alignment)")
        self.pool_scales = tuple(int(s) for s in pool_scales)
        self._init_cls(in_channels, int(channels))
        C = self.channels
        self.psp_modules = nn.ModuleList([nn.Sequential(nn.AdaptiveAvgPool2d(s), _ConvModule(in_channels[-1], C, 1)) for s in self.pool_scales])
        self.bottleneck = _ConvModule(in_channels[-1] + len(self.pool_scales) * C, C, 3)
        self.lateral_convs = nn.ModuleList([_ConvModule(c, C, 1) for c in in_channels[:-1]])
        self.fpn_convs = nn.ModuleList([_ConvModule(C, C, 3) for _ in in_channels[:-1]])
        self.fpn_bottleneck = _ConvModule(len(in_channels) * C, C, 3)
        self.slice_classes = None if slice_classes is None else [int(k) for k in slice_classes]
        for i, k in enumerate(self.slice_classes or []):
            head = nn.Sequential(nn.Dropout2d(0.1), nn.Conv2d(C, k, kernel_size=1))
            setattr(self, "semseghead_%d" % (i + 1), head)

    def trained_parameter_names(self):
        """the parameters a training step updates: with slice_classes the per-slice classifiers replace conv_seg (models.py:129-143, 345-351)"""
        skip = "conv_seg." if self.slice_classes else "semseghead_"
        return [n for n, p in self.named_parameters() if p.requires_grad and not n.startswith(skip)]

    # ------------------------------------------------------------------ fast path
    def loss_and_grads(self, labels, slices=None):
        """-> fn(feats) -> (loss, dfeats): the head's forward, the fused loss and the head's backward without autograd, in
        DataParallelTrainer.step's `loss_and_grads` form.  The head's parameter gradients are accumulated into .grad.
        slices=k (equal parts) or a list of k slice sizes: the trunk runs on each slice separately (BN statistics per slice, models.py:345-351) with classifier semseghead_{i+1}
        (slice_classes); the k losses are summed."""
        nsl = None if slices is None else (len(slices) if isinstance(slices, (list, tuple)) else int(slices))
        if nsl is not None and (self.slice_classes is None or len(self.slice_classes) != nsl):
            raise ValueError("loss_and_grads: %d slices need slice_classes with %d entries" % (nsl, nsl))

        def fn(feats):
            inputs = self._transform_inputs(list(feats))
            self._check_inputs(inputs)
            B = inputs[0].shape[0]
            if isinstance(slices, (list, tuple)):
                sizes = [int(n) for n in slices]
            else:
                k = slices or 1
                if B % k:
                    raise ValueError("batch %d does not split into %d equal slices (pass the slice sizes)" % (B, k))
                sizes = [B // k] * k
            if sum(sizes) != B:
                raise ValueError("slice sizes %s do not add up to the batch %d" % (sizes, B))
            starts = [sum(sizes[:t]) for t in range(len(sizes))]
            G = self._zero_grads()
            dins = [torch.empty(f.shape, device=f.device, dtype=F32) for f in inputs]
            total = torch.zeros((), device=inputs[0].device, dtype=F32)
            for t, (b0, b) in enumerate(zip(starts, sizes)):
                eng = self.engine(self, self.precision)
                xs, shapes = _rows(eng, [f[b0:b0 + b] for f in inputs])
                cls, p = (CLS, None) if slices is None else (("semseghead_%d.1.weight" % (t + 1), "semseghead_%d.1.bias" % (t + 1)), 0.1)
                _, dxs, Gt = self._engine_pass(eng, xs, shapes, labels[b0:b0 + b], total=total, cls=cls, p=p)
                for n in G:
                    G[n] += Gt[n]
                for d, x, shp in zip(dins, dxs, shapes):
                    d[b0:b0 + b] = eng.to_nchw(x, *shp)
            self._accumulate_grads(G, skip={n for n in G if n.startswith("semseghead_" if slices is None else "conv_seg")})
            return total, dins
        return fn
