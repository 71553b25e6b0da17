"""Generate f17_upernet.npz: the reference's own UPerHead (RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/uper_head.py) run in float64.

Runs in the development container only (the reference is not on the GPU machine).  uper_head.py is imported by path; what it imports from mmcv /
mmseg / opencd is not installed, so each of those is restated below from the published algorithm and labelled STUB:
  mmcv.cnn.ConvModule (conv without bias under a norm -> BatchNorm2d 'bn' -> ReLU), mmseg's resize (F.interpolate), PPM (AdaptiveAvgPool2d -> ConvModule
  1x1 per scale, each resized to the input), BaseDecodeHead (the 'multiple_select' input transform, conv_seg, Dropout2d, cls_seg, loss_by_feat with
  CrossEntropyLoss(use_sigmoid=False, avg_non_ignore=False): logits resized to the labels, the per-pixel loss summed and divided by ALL pixels).
Dropout2d is fed an explicit (N, C) mask so the run is reproducible.  Recorded, for a reduced head (in_channels 16/24/32/48, channels 8, 5 classes,
batch 4) at two geometries (maps 16/8/4/2 and 20/10/5/3): the initial state (seeded weights, non-trivial BN statistics), inputs, labels with ignored
pixels (inputs rounded to float16, stored so), the mask; the training-mode logits, loss, d(inputs), every parameter gradient and the updated running statistics; the eval-mode logits from
the initial state (one initial state for both geometries).  The data seed is the first whose BatchNorm outputs all keep 2e-5 away from
the ReLU's kink, so that a float32 run takes the same branch everywhere.  And the reference head's ordered state-dict (key, shape) list at the loveda config's sizes.

    python tests/golden/make_upernet.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/uper_head.py"


# ---------------------------------------------------------------------------------------------------------------- STUBS
def resize(input, size=None, scale_factor=None, mode="nearest", align_corners=None, warning=True):
    """STUB of mmseg.models.utils.resize: F.interpolate"""
    return F.interpolate(input, size, scale_factor, mode, align_corners)


class ConvModule(nn.Module):
    """STUB of mmcv.cnn.ConvModule, order ('conv', 'norm', 'act'), bias='auto' (no conv bias when there is a norm)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias="auto", conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type="ReLU"), inplace=True, **kw):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias=norm_cfg is None if bias == "auto" else bias)
        if norm_cfg is not None:
            self.bn = nn.BatchNorm2d(out_channels)     # BN and SyncBN alike are named 'bn' by mmcv's build_norm_layer
        self.act = nn.ReLU() if act_cfg is not None else None

    def forward(self, x):
        x = self.conv(x)
        if hasattr(self, "bn"):
            x = self.bn(x)
        return self.act(x) if self.act is not None else x


class PPM(nn.ModuleList):
    """STUB of mmseg.models.decode_heads.psp_head.PPM"""

    def __init__(self, pool_scales, in_channels, channels, conv_cfg, norm_cfg, act_cfg, align_corners, **kwargs):
        super().__init__()
        self.align_corners = align_corners
        for s in pool_scales:
            self.append(nn.Sequential(nn.AdaptiveAvgPool2d(s), ConvModule(in_channels, channels, 1, conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg)))

    def forward(self, x):
        return [resize(ppm(x), size=x.size()[2:], mode="bilinear", align_corners=self.align_corners) for ppm in self]


class MaskDropout2d(nn.Module):
    """Dropout2d with the mask set from outside (0 or 1 / (1 - p) per sample and channel)"""
    mask = None

    def forward(self, x):
        return x if MaskDropout2d.mask is None else x * MaskDropout2d.mask[:, :, None, None]


class BaseDecodeHead(nn.Module):
    """STUB of mmseg 1.x BaseDecodeHead: what UPerHead uses"""

    def __init__(self, in_channels, channels, *, num_classes, dropout_ratio=0.1, conv_cfg=None, norm_cfg=None, act_cfg=dict(type="ReLU"), in_index=-1,
                 input_transform=None, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), ignore_index=255,
                 align_corners=False, init_cfg=None, **kw):
        super().__init__()
        self.in_channels, self.channels, self.num_classes = in_channels, channels, num_classes
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        self.in_index, self.input_transform = in_index, input_transform
        self.ignore_index, self.align_corners = ignore_index, align_corners
        self.loss_weight = loss_decode.get("loss_weight", 1.0)
        self.conv_seg = nn.Conv2d(channels, num_classes, kernel_size=1)
        self.dropout = MaskDropout2d() if dropout_ratio > 0 else None

    def _transform_inputs(self, inputs):
        assert self.input_transform == "multiple_select"
        return [inputs[i] for i in self.in_index]

    def cls_seg(self, feat):
        if self.dropout is not None:
            feat = self.dropout(feat)
        return self.conv_seg(feat)

    def loss_by_feat(self, seg_logits, seg_label):
        seg_logits = resize(seg_logits, size=seg_label.shape[1:], mode="bilinear", align_corners=self.align_corners)
        loss = F.cross_entropy(seg_logits, seg_label.long(), reduction="none", ignore_index=self.ignore_index)
        return self.loss_weight * loss.sum() / loss.numel()


def _install_stubs():
    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    class _Reg:
        def register_module(self, *a, **k):
            return lambda cls: cls
    mod("mmcv"), mod("mmcv.cnn", ConvModule=ConvModule)
    mod("opencd"), mod("opencd.registry", MODELS=_Reg())
    mod("mmseg"), mod("mmseg.models"), mod("mmseg.models.utils", resize=resize)
    mod("mmseg.models.decode_heads"), mod("mmseg.models.decode_heads.decode_head", BaseDecodeHead=BaseDecodeHead)
    mod("mmseg.models.decode_heads.psp_head", PPM=PPM)


def _load():
    _install_stubs()
    spec = importlib.util.spec_from_file_location("ref_uper_head", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.UPerHead


CFG = dict(in_channels=[16, 24, 32, 48], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=8, dropout_ratio=0.1, num_classes=5,
           norm_cfg=dict(type="BN", requires_grad=True), align_corners=False, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))
LOVEDA = dict(CFG, in_channels=[1024] * 4, channels=512, num_classes=7, norm_cfg=dict(type="SyncBN", requires_grad=True))
GEOMS = {"g16": (16, 8, 4, 2), "g20": (20, 10, 5, 3)}
B = 4


def _init(head, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, t in head.state_dict(keep_vars=True).items():
            if not t.is_floating_point():
                continue
            if n.endswith("conv.weight"):
                t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64) * (2.0 / (t.shape[0] * t.shape[2] * t.shape[3])) ** 0.5)
            elif n == "conv_seg.weight":
                t.copy_(0.05 * torch.randn(t.shape, generator=g, dtype=torch.float64))
            elif n.endswith("bn.weight"):
                t.copy_(1.0 + 0.2 * torch.randn(t.shape, generator=g, dtype=torch.float64))
            elif n.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g, dtype=torch.float64))
            else:       # biases, running means
                t.copy_(0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64))


def _margin(head, ins):
    """min |BN output| over every ConvModule of one training forward (no state kept)"""
    vals = []
    hooks = [m.register_forward_hook(lambda mod, i, o: vals.append(o.detach().abs().min().item())) for m in head.modules() if isinstance(m, nn.BatchNorm2d)]
    state = {k: v.clone() for k, v in head.state_dict().items()}
    with torch.no_grad():
        head.train()
        MaskDropout2d.mask = None
        head(ins)
    head.load_state_dict(state)
    for h in hooks:
        h.remove()
    return min(vals)


def main():
    UPerHead = _load()
    out = {}
    head = UPerHead(**CFG).double()
    _init(head, 100)
    with torch.no_grad():          # the stored (float32) initial state is exactly the one the run starts from
        for v in head.state_dict().values():
            if v.is_floating_point():
                v.copy_(v.float().double())
    init = {k: v.detach().clone() for k, v in head.state_dict().items()}
    for k, v in init.items():
        out["init." + k] = v.numpy()
    for gi, (tag, geom) in enumerate(GEOMS.items()):
        for attempt in range(100):
            g = torch.Generator().manual_seed(200 + gi + 1000 * attempt)
            ins = [torch.randn(B, c, s, s, generator=g).half().double() for c, s in zip(CFG["in_channels"], geom)]
            if _margin(head, ins) > 2e-5:
                break
        lab = torch.randint(0, CFG["num_classes"], (B, 4 * geom[0], 4 * geom[0]), generator=g)
        lab[torch.rand(lab.shape, generator=g) < 0.15] = 255
        mask = (torch.rand(B, CFG["channels"], generator=g, dtype=torch.float64) >= 0.1).double() / 0.9
        head.load_state_dict(init)
        # training mode
        MaskDropout2d.mask = mask
        head.train()
        head.zero_grad(set_to_none=True)
        xi = [x.clone().requires_grad_(True) for x in ins]
        logits = head(xi)
        loss = head.loss_by_feat(logits, lab)
        loss.backward()
        p = tag + "."
        for i, x in enumerate(ins):
            out[p + "input%d" % i] = x.half().numpy()
            out[p + "dinput%d" % i] = xi[i].grad.numpy()
        out[p + "labels"] = lab.to(torch.uint8).numpy()
        out[p + "mask"] = mask.numpy()
        out[p + "logits_train"] = logits.detach().numpy()
        out[p + "loss"] = np.array(loss.item())
        for n, q in head.named_parameters():
            out[p + "grad." + n] = q.grad.clone().numpy()
        for n, b in head.named_buffers():
            out[p + "after." + n] = b.detach().clone().numpy()      # (a copy: the buffers are reset in place below)
        # eval mode from the initial state
        head.load_state_dict(init)
        head.eval()
        MaskDropout2d.mask = None
        with torch.no_grad():
            out[p + "logits_eval"] = head(ins).numpy()
    big = UPerHead(**LOVEDA)
    out["loveda_keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in big.state_dict().items()]))
    # float32 storage keeps the file small; the float64 run's values rounded once (the tests compare at >= 1e-5 relative)
    out = {k: (v.astype(np.float32) if v.dtype == np.float64 and v.ndim > 0 else v) for k, v in out.items()}
    path = os.path.join(HERE, "f17_upernet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
