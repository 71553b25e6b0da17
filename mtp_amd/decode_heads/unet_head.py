"""UNetHead (the reference's change-detection decode head: RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/unet_head.py, a
segmentation-models-pytorch UNet decoder under mmseg's BaseDecodeHead) on the HIP schedule of engine_unet, under BaseDecodeHead.

State-dict keys and shapes are the reference's (`blocks.{i}.conv{1,2}` = nn.Sequential(conv without bias, norm, ReLU)), so its checkpoints load
strictly.  The forward is BaseDecodeHead's torch.autograd.Function over the engine; `loss_and_grads` is the fast path without autograd, and with `fusion=` it
takes the backbone's 2N-batch maps ("from" images first, "to" images last), fuses the pairs with mtp_fuse_pair_fwd and returns 2N-batch gradients.
"""
import torch
import torch.nn as nn

from .. import ops
from ..engine_unet import UNetEngine
from ..registry import MODELS
from .base import F32, BaseDecodeHead, _rows


class _Conv2dReLU(nn.Sequential):
    """the reference's Conv2dReLU with use_batchnorm=True: conv 3x3 without bias -> BatchNorm2d -> ReLU (torch's default inits, as the reference)"""

    def __init__(self, cin, cout):
        super().__init__(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = _Conv2dReLU(cin + cskip, cout)
        self.conv2 = _Conv2dReLU(cout, cout)


@MODELS.register_module()
class UNetHead(BaseDecodeHead):
    """UNetHead(encoder_channels, decoder_channels, n_blocks, use_batchnorm=True, attention_type=None, center=False, norm_cfg, + BaseDecodeHead's
    in_channels, channels, num_classes, in_index, dropout_ratio, align_corners, ignore_index, loss_decode).  precision: 'fp32' or 'bf16'."""

    engine = UNetEngine

    def __init__(self, encoder_channels=None, decoder_channels=None, n_blocks=5, use_batchnorm=True, attention_type=None, center=False,
                 norm_cfg=dict(type="BN", requires_grad=True), in_channels=None, channels=None, num_classes=None, in_index=(0, 1, 2, 3), dropout_ratio=0.1,
                 act_cfg=dict(type="ReLU"), align_corners=False, ignore_index=255,
                 loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), conv_cfg=None, input_transform="multiple_select",
                 precision="fp32", init_cfg=None, **kwargs):
        if center:
            raise NotImplementedError("UNetHead: center=True is not implemented -- the reference's CenterBlock cannot be constructed (it passes norm_cfg "
                                      "positionally into Conv2dReLU) and no change-detection config sets it")
        if attention_type is not None:
            raise NotImplementedError("UNetHead: attention_type=%r is not implemented (no change-detection config uses scSE attention)" % (attention_type,))
        if use_batchnorm is not True:
            raise NotImplementedError("UNetHead: use_batchnorm=%r is not implemented (every config trains with the norm layer)" % (use_batchnorm,))
        super().__init__(num_classes, in_index, dropout_ratio, norm_cfg, act_cfg, align_corners, ignore_index, loss_decode, conv_cfg, input_transform,
                         precision, **kwargs)
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
        self.encoder_channels, self.decoder_channels, self.n_blocks = encoder_channels, decoder_channels, int(n_blocks)
        self._init_cls(in_channels, channels)
        rev = encoder_channels[::-1]
        cin = [rev[0]] + decoder_channels[:-1]
        cskip = (rev[1:] + [0] * n_blocks)[:n_blocks]
        self.center = nn.Identity()
        self.blocks = nn.ModuleList([_DecoderBlock(a, s, o) for a, s, o in zip(cin, cskip, decoder_channels)])

    # ------------------------------------------------------------------ fast path
    def loss_and_grads(self, labels, fusion=None):
        """-> fn(feats) -> (loss, dfeats): forward, fused loss and backward without autograd, in DataParallelTrainer.step's `loss_and_grads` form;
        the head's parameter gradients are accumulated into .grad.  fusion ('abs_diff' | 'diff' | 'sum' | 'concat'): feats are the backbone's maps
        of the 2N-batch cat([img_from, img_to]); the pairs are fused on the way into channels-last rows and dfeats are the 2N-batch gradients."""
        if fusion is not None:
            ops.fuse_policy(fusion)

        def fn(feats):
            inputs = self._transform_inputs(list(feats))
            self._check_inputs(inputs, 2 if fusion == "concat" else 1)
            eng = self.engine(self, self.precision)
            if fusion is None:
                xs, shapes = _rows(eng, inputs)
            else:
                if inputs[0].shape[0] % 2:
                    raise ValueError("UNetHead: fusion needs the 2N-batch ('from' images first, 'to' images last)")
                inputs = [f.contiguous() for f in inputs]
                N = int(inputs[0].shape[0]) // 2
                shapes = [(N, int(f.shape[2]), int(f.shape[3])) for f in inputs]
                xs = [ops.fuse_pair_fwd(f, torch.empty(N * h * w, c, device=f.device, dtype=eng.act), fusion)
                      for f, c, (_, h, w) in zip(inputs, self.in_channels, shapes)]
            loss, dxs, G = self._engine_pass(eng, xs, shapes, labels, self._zero_grads())
            if fusion is None:
                dins = [eng.to_nchw(d, *s) for d, s in zip(dxs, shapes)]
            else:
                dins = [ops.fuse_pair_bwd(d, f, torch.empty(f.shape, device=f.device, dtype=F32), fusion) for d, f in zip(dxs, inputs)]
            self._accumulate_grads(G)
            return loss.clone(), dins
        return fn
