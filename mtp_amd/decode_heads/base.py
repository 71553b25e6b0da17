"""BaseDecodeHead: what mmseg 1.x's BaseDecodeHead is to its heads (config checks, conv_seg + Dropout2d, input selection, loss, predict), and what
the HIP heads share on top of it: one torch.autograd.Function over a schedule of engine_decode, eval-mode logits as channels-last rows, and the
pieces of the `loss_and_grads` fast path.  A head names its schedule in the class attribute `engine` and keeps its own modules and refusals.
"""
import torch
import torch.nn as nn

from .. import ops
from ..engine_decode import F32, DecodeEngine

CLS = ("conv_seg.weight", "conv_seg.bias")


def _params(mod):
    d = dict(mod.named_parameters())
    d.update(dict(mod.named_buffers()))
    return d


def _rows(eng, inputs):
    """NCHW maps -> (channels-last rows in ACT, their (N, H, W))"""
    return [eng.to_rows(f) for f in inputs], [(int(f.shape[0]), int(f.shape[2]), int(f.shape[3])) for f in inputs]


class _HeadFn(torch.autograd.Function):
    """inputs (NCHW) + the head's parameters -> logits on the head's output grid (with_cls) or the trunk's features, NCHW f32"""

    @staticmethod
    def forward(ctx, head, with_cls, mask, n_in, *args):
        inputs = args[:n_in]
        eng = head.engine(head, head.precision)
        xs, shapes = _rows(eng, inputs)
        feat, c = eng.forward_feature(xs, shapes, _params(head), head.training, head._reduce_fn())
        grid, cl = c["grid"], None
        if with_cls:
            logits, grid, cl = eng.logits_fwd(feat, grid, mask, *CLS)
            out = eng.to_nchw(logits, *grid, head.out_channels)
        else:
            out = eng.to_nchw(feat, *grid)
        ctx.state = (head, eng, c, cl, shapes, [f.dtype for f in inputs])
        return out

    @staticmethod
    def backward(ctx, dout):
        head, eng, c, cl, shapes, dts = ctx.state
        ctx.state = None
        G = {n: torch.zeros_like(p) for n, p in head.named_parameters()}
        dfeat = eng.to_rows(dout.float(), F32) if cl is None else eng.logits_bwd(eng.padded_rows(dout), cl, G)
        dxs = eng.backward_feature(dfeat, c, G)
        dins = [eng.to_nchw(d, *s).to(dt) for d, s, dt in zip(dxs, shapes, dts)]
        return (None, None, None, None, *dins, *[G[n] for n, _ in head.named_parameters()])


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, loss_weight):
        N, K, h, w = logits.shape
        loss, dl = ops.seg_ce(DecodeEngine.padded_rows(logits), K, N, h, w, labels.contiguous(), ignore_index, loss_weight)
        ctx.state = (dl, N, K, h, w, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dl, N, K, h, w, dt = ctx.state
        ctx.state = None
        d = ops.tokens_to_nchw(dl, torch.empty(N, dl.shape[1], h, w, device=dl.device, dtype=F32), N, h, w, 0)[:, :K]
        return (d * dloss).to(dt), None, None, None


class BaseDecodeHead(nn.Module):
    """BaseDecodeHead(num_classes, in_index, dropout_ratio, norm_cfg, act_cfg, align_corners, ignore_index, loss_decode, conv_cfg, input_transform,
    precision, sampler=, out_channels=): checks the configuration; the subclass then applies its own channel rules and calls `_init_cls`."""

    engine = None        # the head's schedule: a DecodeEngine subclass

    def __init__(self, num_classes, in_index, dropout_ratio, norm_cfg, act_cfg, align_corners, ignore_index, loss_decode, conv_cfg, input_transform,
                 precision, **kwargs):
        super().__init__()
        me = type(self).__name__
        if align_corners:
            raise NotImplementedError("%s: align_corners=True is not implemented (the HIP resize kernels are align_corners=False)" % me)
        nt = (norm_cfg or {}).get("type", "BN")
        if norm_cfg is None or nt not in ("BN", "SyncBN", "BN2d"):
            raise NotImplementedError("%s: norm_cfg type %r is not implemented (BN | SyncBN)" % (me, None if norm_cfg is None else nt))
        if (act_cfg or {}).get("type", "ReLU") != "ReLU" or act_cfg is None:
            raise NotImplementedError("%s: act_cfg %r is not implemented (ReLU)" % (me, act_cfg))
        ld = loss_decode if isinstance(loss_decode, dict) else None
        lt = None if ld is None else str(ld.get("type", "CrossEntropyLoss"))
        if lt is not None and lt.startswith("mmseg."):
            lt = lt[len("mmseg."):]      # the configs' scoped name of the same loss
        if lt != "CrossEntropyLoss" or ld.get("use_sigmoid", False) or ld.get("use_mask", False) or ld.get("class_weight") is not None \
                or ld.get("avg_non_ignore", False):
            raise NotImplementedError("%s: loss_decode %r is not implemented (CrossEntropyLoss, use_sigmoid=False, no class weights)" % (me, loss_decode))
        if conv_cfg is not None or input_transform != "multiple_select":
            raise NotImplementedError("%s: conv_cfg / input_transform other than the defaults are not implemented" % me)
        if kwargs.get("sampler") is not None or kwargs.get("out_channels", num_classes) != num_classes:
            raise NotImplementedError("%s: samplers and out_channels != num_classes are not implemented" % me)
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        self.sync_bn, self.loss_weight = nt == "SyncBN", float(ld.get("loss_weight", 1.0))
        self.num_classes = self.out_channels = int(num_classes)
        self.in_index = list(in_index)
        self.dropout_ratio = float(dropout_ratio)
        self.norm_cfg, self.act_cfg, self.align_corners = norm_cfg, act_cfg, False
        self.ignore_index = int(ignore_index)
        self.precision = precision
        self.dropout_mask = None        # tests: an explicit (N, channels) Dropout2d mask of 0 and 1 / (1 - p) for the next forward

    def _init_cls(self, in_channels, channels):
        """conv_seg first (the state-dict order), N(0, 0.01) / 0, and the Dropout2d in front of it"""
        self.in_channels, self.channels = in_channels, channels
        self.conv_seg = nn.Conv2d(self.channels, self.out_channels, kernel_size=1)
        nn.init.normal_(self.conv_seg.weight, 0.0, 0.01)
        nn.init.constant_(self.conv_seg.bias, 0.0)
        if self.dropout_ratio > 0:
            self.dropout = nn.Dropout2d(self.dropout_ratio)

    def trained_parameter_names(self):
        """the parameters a training step updates"""
        return [n for n, p in self.named_parameters() if p.requires_grad]

    # ------------------------------------------------------------------ helpers
    def _transform_inputs(self, inputs):
        return [inputs[i] for i in self.in_index]

    def _check_inputs(self, inputs, div=1):
        """div: the maps carry in_channels / div channels each (the halves of fusion='concat')"""
        for f, c in zip(inputs, self.in_channels):
            if f.dim() != 4 or f.shape[1] * div != c:
                raise ValueError("%s: expected NCHW maps with channels %s%s" % (type(self).__name__, self.in_channels, " (halves, fusion='concat')" if div == 2 else ""))

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

    # ------------------------------------------------------------------ mmseg surface
    def _forward_feature(self, inputs):
        """the trunk's output (what cls_seg reads), NCHW f32"""
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
        return dict(loss_ce=_SegLossFn.apply(seg_logits, labels, self.ignore_index, self.loss_weight))

    def loss(self, inputs, labels):
        return self.loss_by_feat(self.forward(inputs), labels)

    @torch.no_grad()
    def predict(self, inputs, size):
        logits = self.forward(inputs)
        N, K, h, w = logits.shape
        H, W = size
        rows = DecodeEngine.padded_rows(logits)
        up = ops.resize_bilinear_fwd(rows, torch.empty(N * H * W, rows.shape[1], device=rows.device, dtype=F32), N, h, w, H, W)
        return DecodeEngine.to_nchw(up, N, H, W, K)

    @torch.no_grad()
    def logit_rows(self, inputs):
        """eval-mode logits as channels-last rows: (logits (N*H*W, Kp) f32 on the head's output grid, columns K .. Kp zero; (N, H, W)) -- the head's
        eval-mode schedule with no NCHW round trip, what the segmentors' encode_decode hands to the inference kernels"""
        inputs = self._transform_inputs(list(inputs))
        self._check_inputs(inputs)
        eng = self.engine(self, self.precision)
        xs, shapes = _rows(eng, inputs)
        feat, c = eng.forward_feature(xs, shapes, _params(self), False, None)
        logits, grid, _ = eng.logits_fwd(feat, c["grid"], None, *CLS)
        return logits, grid

    # ------------------------------------------------------------------ fast path
    def _zero_grads(self):
        return {n: torch.zeros_like(p) for n, p in self.named_parameters()}

    def _engine_pass(self, eng, xs, shapes, labels, G=None, total=None, cls=CLS, p=None):
        """one pass of the schedule without autograd: forward_feature -> logits_fwd (classifier `cls`, Dropout2d ratio p) -> the fused loss ->
        logits_bwd -> backward_feature -> (loss, d(xs) as f32 rows, G).  The parameter gradients overwrite G.  Where the caller's zero fills and
        loss sum are launched is part of what a kernel trace of a training step shows, so each head keeps its own order: G = None allocates the
        gradients after the loss (a slice of UPerHead, which also adds the loss into `total` there), UNetHead hands in the G it zeroed before."""
        P = _params(self)
        feat, c = eng.forward_feature(xs, shapes, P, self.training, self._reduce_fn())
        mask = self._mask(shapes[0][0], self.dropout_ratio if p is None else p, feat.device)
        logits, grid, cl = eng.logits_fwd(feat, c["grid"], mask, *cls)
        loss, dl = ops.seg_ce(logits, P[cls[0]].shape[0], *grid, labels.contiguous(), self.ignore_index, self.loss_weight)
        if total is not None:
            total += loss
        G = self._zero_grads() if G is None else G
        return loss, eng.backward_feature(eng.logits_bwd(dl, cl, G), c, G), G

    def _accumulate_grads(self, G, skip=()):
        """G into the parameters' .grad, except the names in `skip`"""
        for n, prm in self.named_parameters():
            if n in skip:
                continue
            if prm.grad is None:
                prm.grad = G[n]
            else:
                prm.grad.add_(G[n])       # in place: under DataParallelTrainer .grad is a view of the head's flat gradient buffer
