"""UNetHead (the reference's change-detection decode head: RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/unet_head.py, a
segmentation-models-pytorch UNet decoder under mmseg's BaseDecodeHead) on the HIP schedule of engine_unet.

State-dict keys and shapes are the reference's (`blocks.{i}.conv{1,2}` = nn.Sequential(conv without bias, norm, ReLU)), so its checkpoints load
strictly.  The forward is one torch.autograd.Function over the engine; `loss_and_grads` is the fast path without autograd, and with `fusion=` it
takes the backbone's 2N-batch maps ("from" images first, "to" images last), fuses the pairs with mtp_fuse_pair_fwd and returns 2N-batch gradients.
"""
import torch
import torch.nn as nn

from .. import ops
from ..engine_unet import UNetEngine
from ..engine_uper import F32
from ..registry import MODELS
from .uper_head import UPerHead, _check_cfg, _params


class _Conv2dReLU(nn.Sequential):
    """the reference's Conv2dReLU with use_batchnorm=True: conv 3x3 without bias -> BatchNorm2d -> ReLU (torch's default inits, as the reference)"""

    def __init__(self, cin, cout):
        super().__init__(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = _Conv2dReLU(cin + cskip, cout)
        self.conv2 = _Conv2dReLU(cout, cout)


class _UNetFn(torch.autograd.Function):
    """inputs (NCHW) + the parameters -> logits on the 2x grid (with_cls) or the last block's output, NCHW f32"""

    @staticmethod
    def forward(ctx, head, with_cls, mask, n_in, *args):
        inputs = args[:n_in]
        eng = UNetEngine(head, head.precision)
        xs = [eng.to_rows(f) for f in inputs]
        shapes = [(int(f.shape[0]), int(f.shape[2]), int(f.shape[3])) for f in inputs]
        feat, c = eng.forward_feature(xs, shapes, _params(head), head.training, head._reduce_fn())
        N, (h, w) = c["N"], c["grid"]
        cl = None
        if with_cls:
            up, cl = eng.logits_fwd(feat, N, h, w, mask)
            out = eng.to_nchw(up, N, 2 * h, 2 * w, head.out_channels)
        else:
            out = eng.to_nchw(feat, N, h, w)
        ctx.state = (head, eng, c, cl, shapes, [f.dtype for f in inputs])
        return out

    @staticmethod
    def backward(ctx, dout):
        head, eng, c, cl, shapes, dts = ctx.state
        ctx.state = None
        G = {n: torch.zeros_like(p) for n, p in head.named_parameters()}
        N, (h, w) = c["N"], c["grid"]
        if cl is not None:
            Kp = cl["cc"]["Kp"]
            dl = torch.zeros(N, Kp, 2 * h, 2 * w, device=dout.device, dtype=F32)
            dl[:, :cl["cc"]["K"]] = dout
            dfeat = eng.logits_bwd(eng.to_rows(dl, F32), cl, G)
        else:
            dfeat = eng.to_rows(dout.float().contiguous(), F32)
        dxs = eng.backward_feature(dfeat, c, G)
        dins = [eng.to_nchw(d, n, hh, ww).to(dt) for d, (n, hh, ww), dt in zip(dxs, shapes, dts)]
        return (None, None, None, None, *dins, *[G[n] for n, _ in head.named_parameters()])


@MODELS.register_module()
class UNetHead(nn.Module):
    """UNetHead(encoder_channels, decoder_channels, n_blocks, use_batchnorm=True, attention_type=None, center=False, norm_cfg, + BaseDecodeHead's
    in_channels, channels, num_classes, in_index, dropout_ratio, align_corners, ignore_index, loss_decode).  precision: 'fp32' or 'bf16'."""

    def __init__(self, encoder_channels=None, decoder_channels=None, n_blocks=5, use_batchnorm=True, attention_type=None, center=False,
                 norm_cfg=dict(type="BN", requires_grad=True), in_channels=None, channels=None, num_classes=None, in_index=(0, 1, 2, 3), dropout_ratio=0.1,
                 act_cfg=dict(type="ReLU"), align_corners=False, ignore_index=255,
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), conv_cfg=None, input_transform="multiple_select",
                 precision="fp32", init_cfg=None, **kwargs):
        super().__init__()
        if center:
            raise NotImplementedError("UNetHead: center=True is not implemented -- the reference's CenterBlock cannot be constructed (it passes norm_cfg "
                                      "positionally into Conv2dReLU) and no change-detection config sets it")
        if attention_type is not None:
            raise NotImplementedError("UNetHead: attention_type=%r is not implemented (no change-detection config uses scSE attention)" % (attention_type,))
        if use_batchnorm is not True:
            raise NotImplementedError("UNetHead: use_batchnorm=%r is not implemented (every config trains with the norm layer)" % (use_batchnorm,))
        if isinstance(loss_decode, dict) and str(loss_decode.get("type", "")).startswith("mmseg."):
            loss_decode = dict(loss_decode, type=loss_decode["type"][len("mmseg."):])      # the configs' scoped name of the same loss
        self.sync_bn, self.loss_weight = _check_cfg(norm_cfg, act_cfg, align_corners, loss_decode)
        if conv_cfg is not None or input_transform != "multiple_select":
            raise NotImplementedError("UNetHead: conv_cfg / input_transform other than the defaults are not implemented")
        if kwargs.get("sampler") is not None or kwargs.get("out_channels", num_classes) != num_classes:
            raise NotImplementedError("UNetHead: samplers and out_channels != num_classes are not implemented")
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        encoder_channels, decoder_channels = [int(c) for c in encoder_channels], [int(c) for c in decoder_channels]
        if n_blocks != len(decoder_channels):
            raise ValueError("Model depth is {}, but you provide `decoder_channels` for {} blocks.".format(n_blocks, len(decoder_channels)))
        if n_blocks < len(encoder_channels) - 1:
            raise NotImplementedError("UNetHead: fewer blocks than skips (an encoder map no block reads) is not implemented")
        in_channels = encoder_channels if in_channels is None else [int(c) for c in in_channels]
        channels = decoder_channels[-1] if channels is None else int(channels)
        if in_channels != encoder_channels or channels != decoder_channels[-1]:
            raise ValueError("UNetHead: in_channels must equal encoder_channels and channels must equal decoder_channels[-1]")
        if any(c % 8 for c in encoder_channels + decoder_channels):
            raise NotImplementedError("UNetHead: encoder_channels and decoder_channels must be multiples of 8 (the GEMMs' operand alignment)")
        self.in_channels, self.channels, self.num_classes = in_channels, channels, int(num_classes)
        self.out_channels = self.num_classes
        self.in_index = list(in_index)
        self.encoder_channels, self.decoder_channels, self.n_blocks = encoder_channels, decoder_channels, int(n_blocks)
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
        rev = encoder_channels[::-1]
        cin = [rev[0]] + decoder_channels[:-1]
        cskip = (rev[1:] + [0] * n_blocks)[:n_blocks]
        self.center = nn.Identity()
        self.blocks = nn.ModuleList([_DecoderBlock(a, s, o) for a, s, o in zip(cin, cskip, decoder_channels)])

    def trained_parameter_names(self):
        return [n for n, p in self.named_parameters() if p.requires_grad]

    # ------------------------------------------------------------------ helpers shared with UPerHead (the BaseDecodeHead half)
    _transform_inputs = UPerHead._transform_inputs
    _reduce_fn = UPerHead._reduce_fn
    _mask = UPerHead._mask
    cls_seg = UPerHead.cls_seg
    loss_by_feat = UPerHead.loss_by_feat
    loss = UPerHead.loss
    predict = UPerHead.predict

    def _check_inputs(self, inputs, fusion=None):
        k = 2 if fusion == "concat" else 1
        for f, c in zip(inputs, self.in_channels):
            if f.dim() != 4 or f.shape[1] * k != c:
                raise ValueError("UNetHead: expected NCHW maps with channels %s%s" % (self.in_channels, " (halves, fusion='concat')" if k == 2 else ""))
        if fusion is not None and inputs[0].shape[0] % 2:
            raise ValueError("UNetHead: fusion needs the 2N-batch ('from' images first, 'to' images last)")

    # ------------------------------------------------------------------ mmseg surface
    def _forward_feature(self, inputs):
        """the last decoder block's output (before the final x2 resize and cls_seg), NCHW f32"""
        inputs = self._transform_inputs(inputs)
        self._check_inputs(inputs)
        return _UNetFn.apply(self, False, None, len(inputs), *inputs, *self.parameters())

    def forward(self, inputs):
        inputs = self._transform_inputs(inputs)
        self._check_inputs(inputs)
        mask = self._mask(inputs[0].shape[0], self.dropout_ratio, inputs[0].device)
        return _UNetFn.apply(self, True, mask, len(inputs), *inputs, *self.parameters())

    @torch.no_grad()
    def logit_rows(self, inputs):
        """eval-mode logits as channels-last rows: (logits (N*H*W, Kp) f32 on the head's output grid, columns K .. Kp zero; (N, H, W)) -- what
        SiamEncoderDecoder.encode_decode hands to the inference kernels"""
        inputs = self._transform_inputs(list(inputs))
        self._check_inputs(inputs)
        eng = UNetEngine(self, self.precision)
        xs = [eng.to_rows(f) for f in inputs]
        shapes = [(int(f.shape[0]), int(f.shape[2]), int(f.shape[3])) for f in inputs]
        feat, c = eng.forward_feature(xs, shapes, _params(self), False, None)
        N, (h, w) = c["N"], c["grid"]
        up, _ = eng.logits_fwd(feat, N, h, w, None)
        return up, (N, 2 * h, 2 * w)

    # ------------------------------------------------------------------ fast path
    def loss_and_grads(self, labels, fusion=None):
        """-> fn(feats) -> (loss, dfeats): forward, fused loss and backward without autograd, in DataParallelTrainer.step's `loss_and_grads` form;
        the head's parameter gradients are accumulated into .grad.  fusion ('abs_diff' | 'diff' | 'sum' | 'concat'): feats are the backbone's maps
        of the 2N-batch cat([img_from, img_to]); the pairs are fused on the way into channels-last rows and dfeats are the 2N-batch gradients."""
        if fusion is not None:
            ops.fuse_policy(fusion)

        def fn(feats):
            inputs = self._transform_inputs(list(feats))
            self._check_inputs(inputs, fusion)
            eng = UNetEngine(self, self.precision)
            if fusion is None:
                xs = [eng.to_rows(f) for f in inputs]
                N = int(inputs[0].shape[0])
            else:
                eng.dev = inputs[0].device
                inputs = [f.contiguous() for f in inputs]
                N = int(inputs[0].shape[0]) // 2
                xs = [ops.fuse_pair_fwd(f, eng._e(N * f.shape[2] * f.shape[3], c), fusion) for f, c in zip(inputs, self.in_channels)]
            shapes = [(N, int(f.shape[2]), int(f.shape[3])) for f in inputs]
            G = {n: torch.zeros_like(p) for n, p in self.named_parameters()}
            feat, c = eng.forward_feature(xs, shapes, _params(self), self.training, self._reduce_fn())
            _, (h, w) = c["N"], c["grid"]
            up, cl = eng.logits_fwd(feat, N, h, w, self._mask(N, self.dropout_ratio, feat.device))
            loss, dup = ops.seg_ce(up, self.out_channels, N, 2 * h, 2 * w, labels.contiguous(), self.ignore_index, self.loss_weight)
            dxs = eng.backward_feature(eng.logits_bwd(dup, cl, G), c, G)
            if fusion is None:
                dins = [eng.to_nchw(d, n, hh, ww) for d, (n, hh, ww) in zip(dxs, shapes)]
            else:
                dins = [ops.fuse_pair_bwd(d, f, torch.empty(f.shape, device=f.device, dtype=F32), fusion) for d, f in zip(dxs, inputs)]
            for n, prm in self.named_parameters():
                if prm.grad is None:
                    prm.grad = G[n]
                else:
                    prm.grad.add_(G[n])       # in place: under DataParallelTrainer .grad is a view of the head's flat gradient buffer
            return loss.clone(), dins
        return fn
