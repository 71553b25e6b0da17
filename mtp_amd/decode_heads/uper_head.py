"""UPerHead (mmseg 1.x UPerHead / BaseDecodeHead surface, as the reference uses it: RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/
uper_head.py, the semantic-segmentation configs, Multi-Task_Pretrain/models.py:112-143) on the HIP schedule of engine_uper.

State-dict keys and shapes are mmcv / mmseg's (ConvModule = conv without bias -> bn -> ReLU), so an mmseg checkpoint loads strictly.  The forward
runs through torch.autograd.Functions that call the engine, so the head trains under plain autograd; `loss_and_grads` is the fast path that runs
forward, loss and backward without autograd.
"""
import math

import torch
import torch.nn as nn

from .. import ops
from ..engine_uper import F32, UperEngine
from ..registry import MODELS


class _ConvModule(nn.Module):
    """mmcv ConvModule(conv -> bn -> ReLU), bias='auto' = no conv bias under a norm; init as mmcv (kaiming fan_out relu, BN 1 / 0)"""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        nn.init.kaiming_normal_(self.conv.weight, a=0, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.bn.weight, 1.0)
        nn.init.constant_(self.bn.bias, 0.0)


def _check_cfg(norm_cfg, act_cfg, align_corners, loss_decode):
    if align_corners:
        raise NotImplementedError("UPerHead: align_corners=True is not implemented (the HIP resize kernels are align_corners=False)")
    nt = (norm_cfg or {}).get("type", "BN")
    if norm_cfg is None or nt not in ("BN", "SyncBN", "BN2d"):
        raise NotImplementedError("UPerHead: norm_cfg type %r is not implemented (BN | SyncBN)" % (None if norm_cfg is None else nt))
    if (act_cfg or {}).get("type", "ReLU") != "ReLU" or act_cfg is None:
        raise NotImplementedError("UPerHead: act_cfg %r is not implemented (ReLU)" % (act_cfg,))
    ld = loss_decode if isinstance(loss_decode, dict) else None
    if ld is None or ld.get("type", "CrossEntropyLoss") != "CrossEntropyLoss" or ld.get("use_sigmoid", False) or ld.get("use_mask", False) \
            or ld.get("class_weight") is not None or ld.get("avg_non_ignore", False):
        raise NotImplementedError("UPerHead: loss_decode %r is not implemented (CrossEntropyLoss, use_sigmoid=False, no class weights)" % (loss_decode,))
    return nt == "SyncBN", float(ld.get("loss_weight", 1.0))


def _params(mod):
    d = dict(mod.named_parameters())
    d.update(dict(mod.named_buffers()))
    return d


class _HeadFn(torch.autograd.Function):
    """inputs (NCHW) + the trunk's / classifier's parameters -> logits (with_cls) or the trunk's features, NCHW f32"""

    @staticmethod
    def forward(ctx, head, with_cls, mask, n_in, *args):
        inputs = args[:n_in]
        eng = UperEngine(head, head.precision)
        P = _params(head)
        xs = [eng.to_rows(f) for f in inputs]
        shapes = [(int(f.shape[0]), int(f.shape[2]), int(f.shape[3])) for f in inputs]
        feat, c = eng.forward_feature(xs, shapes, P, head.training, head._reduce_fn())
        N, H0, W0 = shapes[0]
        cc = None
        if with_cls:
            logits, cc = eng.cls_fwd(feat, N, H0 * W0, "conv_seg.weight", "conv_seg.bias", mask)
            out = eng.to_nchw(logits, N, H0, W0, cc["K"])
        else:
            out = eng.to_nchw(feat, N, H0, W0)
        ctx.state = (head, eng, c, cc, shapes, [f.dtype for f in inputs], n_in)
        return out

    @staticmethod
    def backward(ctx, dout):
        head, eng, c, cc, shapes, dts, n_in = ctx.state
        ctx.state = None
        G = {n: torch.zeros_like(p) for n, p in head.named_parameters()}
        N, H0, W0 = shapes[0]
        if cc is not None:
            Kp = cc["Kp"]
            dl = torch.zeros(N, Kp, H0, W0, device=dout.device, dtype=F32)
            dl[:, :cc["K"]] = dout
            dfeat = eng.cls_bwd(eng.to_rows(dl, F32), cc, G, "conv_seg.weight", "conv_seg.bias")
        else:
            dfeat = eng.to_rows(dout.float(), F32)
        dxs = eng.backward_feature(dfeat, c, G)
        dins = [eng.to_nchw(d, N, h, w).to(dt) for d, (N, h, w), dt in zip(dxs, shapes, dts)]
        names = [n for n, _ in head.named_parameters()]
        return (None, None, None, None, *dins, *[G[n] if n in G else None for n in names])


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, loss_weight, precision):
        N, K, h, w = logits.shape
        Kp = ops.pad8(K)
        lp = torch.zeros(N, Kp, h, w, device=logits.device, dtype=F32)
        lp[:, :K] = logits
        rows = ops.nchw_to_tokens(lp, torch.empty(N * h * w, Kp, device=logits.device, dtype=F32), N, h, w, 0)
        loss, dl = ops.seg_ce(rows, K, N, h, w, labels.contiguous(), ignore_index, loss_weight)
        ctx.state = (dl, N, K, h, w, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dl, N, K, h, w, dt = ctx.state
        ctx.state = None
        d = ops.tokens_to_nchw(dl, torch.empty(N, dl.shape[1], h, w, device=dl.device, dtype=F32), N, h, w, 0)[:, :K]
        return (d * dloss).to(dt), None, None, None, None


@MODELS.register_module()
class UPerHead(nn.Module):
    """mmseg UPerHead(pool_scales, in_channels, channels, num_classes, in_index, dropout_ratio, norm_cfg, act_cfg, align_corners, ignore_index,
    loss_decode).  precision: 'fp32' (f32 GEMM operands) or 'bf16'.  slice_classes: the MTP pretraining arrangement (Multi-Task_Pretrain/models.py:
    129-143) -- one Dropout2d(0.1) + Conv2d(channels, classes_i, 1) classifier per dataset slice (semseghead_{1,2,3}), used by loss_and_grads(slices=3)."""

    def __init__(self, in_channels, channels, num_classes, pool_scales=(1, 2, 3, 6), in_index=(0, 1, 2, 3), dropout_ratio=0.1,
                 norm_cfg=dict(type="BN", requires_grad=True), act_cfg=dict(type="ReLU"), align_corners=False, ignore_index=255,
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), conv_cfg=None, input_transform="multiple_select",
                 precision="fp32", slice_classes=None, init_cfg=None, **kwargs):
        super().__init__()
        self.sync_bn, self.loss_weight = _check_cfg(norm_cfg, act_cfg, align_corners, loss_decode)
        if conv_cfg is not None or input_transform != "multiple_select":
            raise NotImplementedError("UPerHead: conv_cfg / input_transform other than the defaults are not implemented")
        if kwargs.get("sampler") is not None or kwargs.get("out_channels", num_classes) != num_classes:
            raise NotImplementedError("UPerHead: samplers and out_channels != num_classes are not implemented")
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        in_channels = list(in_channels)
        if channels % 8 or any(c % 8 for c in in_channels):
            raise NotImplementedError("UPerHead: channels and in_channels must be multiples of 8 (the GEMMs' operand alignment)")
        self.in_channels, self.channels, self.num_classes = in_channels, int(channels), int(num_classes)
        self.out_channels = self.num_classes
        self.in_index = list(in_index)
        self.pool_scales = tuple(int(s) for s in pool_scales)
        self.dropout_ratio = float(dropout_ratio)
        self.norm_cfg, self.act_cfg, self.align_corners = norm_cfg, act_cfg, False
        self.ignore_index = int(ignore_index)
        self.precision = precision
        self.dropout_mask = None        # tests: an explicit (N, channels) Dropout2d mask of 0 and 1 / (1 - p) for the next forward
        # BaseDecodeHead: conv_seg first (the state-dict order), N(0, 0.01) / 0
        self.conv_seg = nn.Conv2d(self.channels, self.out_channels, kernel_size=1)
        nn.init.normal_(self.conv_seg.weight, 0.0, 0.01)
        nn.init.constant_(self.conv_seg.bias, 0.0)
        if self.dropout_ratio > 0:
            self.dropout = nn.Dropout2d(self.dropout_ratio)
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

    # ------------------------------------------------------------------ helpers
    def _transform_inputs(self, inputs):
        return [inputs[i] for i in self.in_index]

    def _reduce_fn(self):
        if not self.sync_bn or not torch.distributed.is_available() or not torch.distributed.is_initialized() \
                or torch.distributed.get_world_size() == 1:
            return getattr(self, "bn_reduce", None)      # bn_reduce: a test hook emulating the exchange
        import torch.distributed as dist

        def red(t):
            dist.all_reduce(t)
            return t
        return red

    def _mask(self, N, p, device):
        if not self.training or p <= 0:
            return None
        if self.dropout_mask is not None:
            m, self.dropout_mask = self.dropout_mask, None
            return m.to(device=device, dtype=F32).contiguous()
        return ((torch.rand(N, self.channels, device=device) >= p).to(F32) / (1.0 - p)).contiguous()

    def _check_inputs(self, inputs):
        for f, c in zip(inputs, self.in_channels):
            if f.dim() != 4 or f.shape[1] != c:
                raise ValueError("UPerHead: expected NCHW maps with channels %s" % self.in_channels)

    # ------------------------------------------------------------------ mmseg surface
    def _forward_feature(self, inputs):
        inputs = self._transform_inputs(inputs)
        self._check_inputs(inputs)
        return _HeadFn.apply(self, False, None, len(inputs), *inputs, *self.parameters())

    def forward(self, inputs):
        inputs = self._transform_inputs(inputs)
        self._check_inputs(inputs)
        mask = self._mask(inputs[0].shape[0], self.dropout_ratio, inputs[0].device)
        return _HeadFn.apply(self, True, mask, len(inputs), *inputs, *self.parameters())

    def cls_seg(self, feat):
        """Dropout2d + conv_seg on an NCHW feature map (torch's own 1x1 conv here: the fused path is forward())"""
        if self.dropout_ratio > 0:
            feat = self.dropout(feat)
        return self.conv_seg(feat)

    def loss_by_feat(self, seg_logits, labels):
        """labels (B, H, W) uint8 / int64 instead of SegDataSamples -> dict(loss_ce=...)"""
        if labels.dim() == 4:
            labels = labels.squeeze(1)
        return dict(loss_ce=_SegLossFn.apply(seg_logits, labels, self.ignore_index, self.loss_weight, self.precision))

    def loss(self, inputs, labels):
        return self.loss_by_feat(self.forward(inputs), labels)

    @torch.no_grad()
    def predict(self, inputs, size):
        logits = self.forward(inputs)
        N, K, h, w = logits.shape
        H, W = size
        Kp = ops.pad8(K)
        lp = torch.zeros(N, Kp, h, w, device=logits.device, dtype=F32)
        lp[:, :K] = logits
        rows = ops.nchw_to_tokens(lp, torch.empty(N * h * w, Kp, device=lp.device, dtype=F32), N, h, w, 0)
        up = ops.resize_bilinear_fwd(rows, torch.empty(N * H * W, Kp, device=lp.device, dtype=F32), N, h, w, H, W)
        return ops.tokens_to_nchw(up, torch.empty(N, Kp, H, W, device=lp.device, dtype=F32), N, H, W, 0)[:, :K].contiguous()

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
            P = _params(self)
            G = {n: torch.zeros_like(p) for n, p in self.named_parameters()}
            dins = [torch.empty(f.shape, device=f.device, dtype=F32) for f in inputs]
            total = torch.zeros((), device=inputs[0].device, dtype=F32)
            for t, (b0, b) in enumerate(zip(starts, sizes)):
                sl = [f[b0:b0 + b] for f in inputs]
                eng = UperEngine(self, self.precision)
                xs = [eng.to_rows(f) for f in sl]
                shapes = [(b, int(f.shape[2]), int(f.shape[3])) for f in sl]
                feat, c = eng.forward_feature(xs, shapes, P, self.training, self._reduce_fn())
                N, H0, W0 = shapes[0]
                wn, bn = ("conv_seg.weight", "conv_seg.bias") if slices is None else ("semseghead_%d.1.weight" % (t + 1), "semseghead_%d.1.bias" % (t + 1))
                p = self.dropout_ratio if slices is None else 0.1
                logits, cc = eng.cls_fwd(feat, N, H0 * W0, wn, bn, self._mask(N, p, feat.device))
                loss, dl = ops.seg_ce(logits, cc["K"], N, H0, W0, labels[b0:b0 + b].contiguous(), self.ignore_index, self.loss_weight)
                total += loss
                Gt = {n: torch.zeros_like(g) for n, g in G.items()}
                dfeat = eng.cls_bwd(dl, cc, Gt, wn, bn)
                dxs = eng.backward_feature(dfeat, c, Gt)
                for n in G:
                    G[n] += Gt[n]
                for d, x, (Nn, h, w) in zip(dins, dxs, shapes):
                    d[b0:b0 + b] = eng.to_nchw(x, Nn, h, w)
            for n, prm in self.named_parameters():
                if n.startswith("semseghead_") and slices is None or (slices is not None and n.startswith("conv_seg")):
                    continue
                if prm.grad is None:
                    prm.grad = G[n]
                else:
                    prm.grad.add_(G[n])       # in place: under DataParallelTrainer .grad is a view of the head's flat gradient buffer
            return total, dins
        return fn
