"""Generate f19_unet.npz: the reference's own UNetHead (RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/unet_head.py) run in float64.

Runs in the development container only (the reference is not on the GPU machine).  unet_head.py is imported by path; what it imports from mmcv /
mmseg / opencd is not installed, so each of those is restated below from the published algorithm and labelled STUB: BaseDecodeHead (as in
make_upernet.py: conv_seg, Dropout2d, cls_seg, loss_by_feat with CrossEntropyLoss(use_sigmoid=False, avg_non_ignore=False)), mmcv's build_norm_layer
(-> BatchNorm2d) and the two registries.  Dropout2d is fed an explicit (N, C) mask.  Recorded, for a reduced head (decoder_channels 32/16/8/8,
channels 8, 2 classes, batch 2, dropout 0.1) at two geometries -- 'flat': four 16-channel maps all 2x3 (the ViT arrangement; logits 64x96 for
32x48 labels, the loss's resize shrinks them); 'pyr': 8/16/24/32 channels at 8x12, 4x6, 2x3, 1x2 (skips that need a real resize; labels of the
logits' size) -- the initial state (seeded weights, non-trivial BN statistics; one per geometry, the channel counts differ), the inputs (rounded to
float16, stored so), labels with ignored pixels, the mask; training-mode logits, loss, d(inputs), every parameter gradient, the updated running
statistics; eval-mode logits from the initial state.  The data seed is the first whose BatchNorm outputs all keep 2e-5 away from the ReLU's kink.
And the reference head's ordered state-dict (key, shape) list at the Levir ViT-L config's sizes.

    python tests/golden/make_unet.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_upernet import BaseDecodeHead, MaskDropout2d      # noqa: E402  STUB of mmseg 1.x BaseDecodeHead (and the explicit-mask Dropout2d)

REF = "/root/reference/RS_Tasks_Finetune/Change_Detection/opencd/models/decode_heads/unet_head.py"


def build_norm_layer(cfg, num_features):
    """STUB of mmcv.cnn.bricks.norm.build_norm_layer for BN / SyncBN: (name, BatchNorm2d)"""
    assert cfg["type"] in ("BN", "SyncBN")
    return "bn", nn.BatchNorm2d(num_features)


def _load():
    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    class _Reg:
        """STUB of the mmseg / opencd MODELS registries"""
        def register_module(self, *a, **k):
            return lambda cls: cls
    mod("mmseg"), mod("mmseg.registry", MODELS=_Reg())
    mod("mmseg.models"), mod("mmseg.models.decode_heads"), mod("mmseg.models.decode_heads.decode_head", BaseDecodeHead=BaseDecodeHead)
    mod("mmcv"), mod("mmcv.cnn"), mod("mmcv.cnn.bricks"), mod("mmcv.cnn.bricks.norm", build_norm_layer=build_norm_layer)
    mod("opencd"), mod("opencd.registry", MODELS=_Reg())
    spec = importlib.util.spec_from_file_location("ref_unet_head", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.UNetHead


HEAD = dict(num_classes=2, channels=8, dropout_ratio=0.1, decoder_channels=[32, 16, 8, 8], n_blocks=4, in_index=[0, 1, 2, 3], use_batchnorm=True,
            center=False, attention_type=None, norm_cfg=dict(type="BN", requires_grad=True), align_corners=False,
            loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))
GEOMS = {"flat": ([16, 16, 16, 16], [(2, 3)] * 4, (32, 48)), "pyr": ([8, 16, 24, 32], [(8, 12), (4, 6), (2, 3), (1, 2)], (32, 64))}
LEVIR = dict(HEAD, channels=64, decoder_channels=[512, 256, 128, 64], in_channels=[1024] * 4, encoder_channels=[1024] * 4,
             norm_cfg=dict(type="SyncBN", requires_grad=True))
B = 2


def _init(head, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, t in head.state_dict(keep_vars=True).items():
            if not t.is_floating_point():
                continue
            if n.endswith(".0.weight"):
                t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64) * (2.0 / (t.shape[0] * 9)) ** 0.5)
            elif n == "conv_seg.weight":
                t.copy_(0.05 * torch.randn(t.shape, generator=g, dtype=torch.float64))
            elif n.endswith(".1.weight"):
                t.copy_(1.0 + 0.2 * torch.randn(t.shape, generator=g, dtype=torch.float64))
            elif n.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g, dtype=torch.float64))
            else:       # biases, running means
                t.copy_(0.1 * torch.randn(t.shape, generator=g, dtype=torch.float64))


def _margin(head, ins):
    """min |BN output| over every Conv2dReLU of one training forward (no state kept)"""
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
    UNetHead = _load()
    out = {}
    for gi, (tag, (chans, sizes, lab_size)) in enumerate(GEOMS.items()):
        head = UNetHead(**dict(HEAD, in_channels=chans, encoder_channels=chans)).double()
        _init(head, 100 + gi)
        with torch.no_grad():          # the stored (float32) initial state is exactly the one the run starts from
            for v in head.state_dict().values():
                if v.is_floating_point():
                    v.copy_(v.float().double())
        init = {k: v.detach().clone() for k, v in head.state_dict().items()}
        p = tag + "."
        for k, v in init.items():
            out[p + "init." + k] = v.numpy()
        for attempt in range(200):
            g = torch.Generator().manual_seed(300 + gi + 1000 * attempt)
            ins = [torch.randn(B, c, *s, generator=g).half().double() for c, s in zip(chans, sizes)]
            if _margin(head, ins) > 2e-5:
                break
        else:
            raise SystemExit("no seed with a ReLU margin")
        lab = torch.randint(0, HEAD["num_classes"], (B,) + lab_size, generator=g)
        lab[torch.rand(lab.shape, generator=g) < 0.15] = 255
        mask = (torch.rand(B, HEAD["channels"], generator=g, dtype=torch.float64) >= 0.1).double() / 0.9
        if bool((mask != 0).all()):      # p = 0.1 on 16 entries: make sure one channel IS dropped
            mask[0, 3] = 0.0
        head.load_state_dict(init)
        MaskDropout2d.mask = mask
        head.train()
        head.zero_grad(set_to_none=True)
        xi = [x.clone().requires_grad_(True) for x in ins]
        logits = head(xi)
        assert tuple(logits.shape[2:]) == (2 * lab_size[0], 2 * lab_size[1]) if tag == "flat" else tuple(logits.shape[2:]) == lab_size
        loss = head.loss_by_feat(logits, lab)
        loss.backward()
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
            out[p + "after." + n] = b.detach().clone().numpy()
        head.load_state_dict(init)
        head.eval()
        MaskDropout2d.mask = None
        with torch.no_grad():
            out[p + "logits_eval"] = head(ins).numpy()
    big = UNetHead(**LEVIR)
    out["levir_keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in big.state_dict().items()]))
    out = {k: (v.astype(np.float32) if v.dtype == np.float64 and v.ndim > 0 else v) for k, v in out.items()}
    path = os.path.join(HERE, "f19_unet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
