"""CPU: the UperNet decode head's module surface (mtp_amd.UPerHead) -- mmseg's state-dict keys, order and shapes, its init, the registry build
from the loveda config's decode_head dict, the configurations that are refused -- and `torch_uper`, the torch restatement of mmseg's UPerHead
forward + loss that the GPU tests (test_hip_uper_head.py) hold the HIP head to."""
import math

import pytest
import torch
import torch.nn.functional as F

import mtp_amd
from mtp_amd import MODELS, UPerHead

# RS_Tasks_Finetune/Semantic_Segmentation/configs/mtp/loveda/rvsa-l-upernet-512-mae-mtp-loveda.py, model.decode_head
LOVEDA = dict(type="UPerHead", in_channels=[1024, 1024, 1024, 1024], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=512,
              dropout_ratio=0.1, num_classes=7, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
              loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))


def mmseg_keys(in_channels, channels, num_classes, pool_scales):
    """mmseg 1.x UPerHead's state-dict order: BaseDecodeHead's conv_seg first, then PPM, bottleneck, lateral / fpn ConvModules, fpn_bottleneck"""
    def cm(pre, cin, cout, k):
        return [(pre + ".conv.weight", (cout, cin, k, k))] + [(pre + ".bn." + n, (cout,)) for n in ("weight", "bias", "running_mean", "running_var")] \
            + [(pre + ".bn.num_batches_tracked", ())]
    keys = [("conv_seg.weight", (num_classes, channels, 1, 1)), ("conv_seg.bias", (num_classes,))]
    for i in range(len(pool_scales)):
        keys += cm("psp_modules.%d.1" % i, in_channels[-1], channels, 1)
    keys += cm("bottleneck", in_channels[-1] + len(pool_scales) * channels, channels, 3)
    for i, c in enumerate(in_channels[:-1]):
        keys += cm("lateral_convs.%d" % i, c, channels, 1)
    for i in range(len(in_channels) - 1):
        keys += cm("fpn_convs.%d" % i, channels, channels, 3)
    keys += cm("fpn_bottleneck", len(in_channels) * channels, channels, 3)
    return keys


# ------------------------------------------------------------------------------------------------ the torch restatement
# probe: when a list, every ConvModule appends min |pre-activation| -- how close the batch comes to the ReLU's kink
probe = None


def _cm(sd, pre, x, training, k):
    x = F.conv2d(x, sd[pre + ".conv.weight"], None, padding=k // 2)
    x = F.batch_norm(x, sd[pre + ".bn.running_mean"], sd[pre + ".bn.running_var"], sd[pre + ".bn.weight"], sd[pre + ".bn.bias"], training, 0.1, 1e-5)
    if probe is not None:
        probe.append(x.detach().abs().min().item())
    return F.relu(x)


def _resize(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def torch_uper_feature(sd, inputs, pool_scales, training):
    """mmseg UPerHead._forward_feature (uper_head.py: psp_forward, laterals, top-down adds, fpn_convs, fpn_bottleneck) with torch ops on the
    state dict `sd` (running statistics updated in place in training mode)"""
    x = inputs[-1]
    psp = [x] + [_resize(_cm(sd, "psp_modules.%d.1" % j, F.adaptive_avg_pool2d(x, s), training, 1), x.shape[2:]) for j, s in enumerate(pool_scales)]
    lat = [_cm(sd, "lateral_convs.%d" % i, inputs[i], training, 1) for i in range(len(inputs) - 1)]
    lat.append(_cm(sd, "bottleneck", torch.cat(psp, 1), training, 3))
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + _resize(lat[i], lat[i - 1].shape[2:])
    outs = [_cm(sd, "fpn_convs.%d" % i, lat[i], training, 3) for i in range(len(lat) - 1)] + [lat[-1]]
    outs = [outs[0]] + [_resize(o, outs[0].shape[2:]) for o in outs[1:]]
    return _cm(sd, "fpn_bottleneck", torch.cat(outs, 1), training, 3)


def torch_uper(sd, inputs, pool_scales, training, mask=None, cls=("conv_seg.weight", "conv_seg.bias")):
    """forward = cls_seg(_forward_feature): Dropout2d as an explicit (N, C) mask of 0 and 1 / (1 - p)"""
    f = torch_uper_feature(sd, inputs, pool_scales, training)
    if mask is not None:
        f = f * mask[:, :, None, None]
    return F.conv2d(f, sd[cls[0]], sd[cls[1]])


def torch_seg_loss(logits, labels, ignore_index=255, loss_weight=1.0):
    """BaseDecodeHead.loss_by_feat: resize the logits to the labels, CrossEntropyLoss(avg_non_ignore=False) = sum over kept pixels / all pixels"""
    up = _resize(logits, labels.shape[1:])
    return loss_weight * F.cross_entropy(up, labels.long(), ignore_index=ignore_index, reduction="sum") / labels.numel()


def small_head(seed=0, **kw):
    torch.manual_seed(seed)
    cfg = dict(in_channels=[32, 48, 64, 96], channels=16, num_classes=5)
    cfg.update(kw)
    return UPerHead(**cfg)


def randomise_bn(head, seed=1):
    """non-trivial affine parameters and running statistics"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, t in head.state_dict(keep_vars=True).items():
            if n.endswith("bn.weight"):
                t.copy_(1.0 + 0.2 * torch.randn(t.shape, generator=g))
            elif n.endswith("bn.bias") or n.endswith("running_mean"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
            elif n.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif n == "conv_seg.bias":
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
    return head


# ------------------------------------------------------------------------------------------------ tests
def test_state_dict_keys_order_and_shapes_match_mmseg():
    for cfg in (dict(in_channels=[32, 48, 64, 96], channels=16, num_classes=5, pool_scales=(1, 2, 3, 6)),
                dict(in_channels=[1024] * 4, channels=512, num_classes=7, pool_scales=(1, 2, 3, 6))):
        h = UPerHead(**cfg)
        got = [(k, tuple(v.shape)) for k, v in h.state_dict().items()]
        assert got == mmseg_keys(cfg["in_channels"], cfg["channels"], cfg["num_classes"], cfg["pool_scales"])


def test_registry_builds_the_loveda_decode_head():
    h = MODELS.build(dict(LOVEDA))
    assert isinstance(h, UPerHead) and h.sync_bn and h.num_classes == 7 and h.channels == 512 and h.in_index == [0, 1, 2, 3]
    assert mtp_amd.UPerHead is UPerHead
    assert h.bottleneck.conv.weight.shape == (512, 1024 + 4 * 512, 3, 3) and h.bottleneck.conv.bias is None


def test_init_follows_mmcv_and_mmseg():
    h = UPerHead(in_channels=[64, 64, 64, 64], channels=128, num_classes=7)
    w = h.conv_seg.weight
    assert abs(w.std().item() - 0.01) < 0.002 and h.conv_seg.bias.abs().max() == 0
    fan_out = 128 * 9
    assert abs(h.fpn_convs[0].conv.weight.std().item() - math.sqrt(2.0 / fan_out)) < 0.05 * math.sqrt(2.0 / fan_out)
    assert (h.bottleneck.bn.weight == 1).all() and (h.bottleneck.bn.bias == 0).all()


@pytest.mark.parametrize("bad", [dict(align_corners=True), dict(norm_cfg=dict(type="GN", num_groups=8)), dict(act_cfg=dict(type="GELU")),
                                 dict(loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0)),
                                 dict(loss_decode=dict(type="DiceLoss"))])
def test_unsupported_configurations_raise(bad):
    with pytest.raises(NotImplementedError):
        small_head(**bad)


def test_slice_classifiers_are_models_py_semseg_heads():
    h = small_head(slice_classes=(4, 6, 8))
    sd = h.state_dict()
    for i, k in enumerate((4, 6, 8)):
        assert sd["semseghead_%d.1.weight" % (i + 1)].shape == (k, 16, 1, 1) and sd["semseghead_%d.1.bias" % (i + 1)].shape == (k,)


def test_torch_restatement_matches_mmseg_modules():
    """the restatement against torch's own modules wired as mmseg's UPerHead (nn.BatchNorm2d in training mode, nn.Dropout2d-style mask)"""
    h = randomise_bn(small_head())
    sd = {k: v.clone().double() for k, v in h.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    ins = [torch.randn(2, c, s, s, generator=g, dtype=torch.float64) for c, s in zip(h.in_channels, (20, 10, 5, 3))]
    mods = h.double().train()
    x = ins[-1]
    psp = [x] + [_resize(F.relu(m[1].bn(m[1].conv(m[0](x)))), x.shape[2:]) for m in mods.psp_modules]
    lat = [F.relu(m.bn(m.conv(ins[i]))) for i, m in enumerate(mods.lateral_convs)] + [F.relu(mods.bottleneck.bn(mods.bottleneck.conv(torch.cat(psp, 1))))]
    for i in range(3, 0, -1):
        lat[i - 1] = lat[i - 1] + _resize(lat[i], lat[i - 1].shape[2:])
    outs = [F.relu(m.bn(m.conv(lat[i]))) for i, m in enumerate(mods.fpn_convs)] + [lat[-1]]
    outs = [outs[0]] + [_resize(o, outs[0].shape[2:]) for o in outs[1:]]
    ref = mods.conv_seg(F.relu(mods.fpn_bottleneck.bn(mods.fpn_bottleneck.conv(torch.cat(outs, 1)))))
    got = torch_uper(sd, ins, h.pool_scales, True)
    assert (got - ref).abs().max().item() < 1e-10
    for k, v in h.state_dict().items():
        if "running" in k:
            assert (sd[k] - v).abs().max().item() < 1e-12, k


# ------------------------------------------------------------------------------------------------ fixture f17: the reference's own UPerHead
F17_CFG = dict(in_channels=[16, 24, 32, 48], channels=8, num_classes=5, pool_scales=(1, 2, 3, 6))


def f17_case(golden, tag, dtype=torch.float64):
    """(state dict, inputs, labels, dropout mask) of fixture f17's geometry `tag` ('g16' / 'g20')"""
    d = golden("f17_upernet.npz")
    sd = {k[5:]: torch.from_numpy(v.copy()) for k, v in d.items() if k.startswith("init.")}
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    ins = [torch.from_numpy(d[tag + ".input%d" % i]).to(dtype) for i in range(4)]
    return sd, ins, torch.from_numpy(d[tag + ".labels"]), torch.from_numpy(d[tag + ".mask"]).to(dtype)


def test_f17_key_list_is_the_reference_heads():
    import json
    from conftest import GOLDEN
    import numpy as np
    import os
    ref = json.loads(str(np.load(os.path.join(GOLDEN, "f17_upernet.npz"))["loveda_keys"]))
    h = MODELS.build(dict(LOVEDA))
    assert [[k, list(v.shape)] for k, v in h.state_dict().items()] == ref
    assert [(k, tuple(s)) for k, s in ref] == mmseg_keys([1024] * 4, 512, 7, (1, 2, 3, 6))


@pytest.mark.parametrize("tag", ["g16", "g20"])
def test_torch_restatement_pinned_to_f17(golden, tag):
    """the restatement every GPU parity test uses, against the reference's own UPerHead (fixture f17, float64): training-mode logits, loss, d(inputs),
    every parameter gradient and the updated running statistics; eval-mode logits -- at 1e-5 relative"""
    from conftest import rel_err
    d = golden("f17_upernet.npz")
    sd, ins, lab, mask = f17_case(golden, tag)
    for k in sd:
        sd[k].requires_grad_(sd[k].is_floating_point() and "running" not in k)
    xi = [x.clone().requires_grad_(True) for x in ins]
    logits = torch_uper(sd, xi, F17_CFG["pool_scales"], True, mask)
    loss = torch_seg_loss(logits, lab)
    loss.backward()
    assert rel_err(logits.detach(), torch.from_numpy(d[tag + ".logits_train"])) < 1e-5
    assert abs(loss.item() - float(d[tag + ".loss"])) < 1e-5 * float(d[tag + ".loss"])
    for i, x in enumerate(xi):
        assert rel_err(x.grad, torch.from_numpy(d[tag + ".dinput%d" % i])) < 1e-5
    h = UPerHead(**F17_CFG)
    for n, _ in h.named_parameters():
        assert rel_err(sd[n].grad, torch.from_numpy(d[tag + ".grad." + n])) < 1e-5, n
    for n, _ in h.named_buffers():
        ref = torch.from_numpy(d[tag + ".after." + n])
        if ref.is_floating_point():
            assert rel_err(sd[n].detach(), ref) < 1e-5, n
        else:       # num_batches_tracked: one training forward (F.batch_norm itself does not count)
            assert int(ref) == int(sd[n]) + 1, n
    sde, ins_e, _, _ = f17_case(golden, tag)
    with torch.no_grad():
        ev = torch_uper(sde, ins_e, F17_CFG["pool_scales"], False)
    assert rel_err(ev, torch.from_numpy(d[tag + ".logits_eval"])) < 1e-5
    # and the module loads the reference's state dict strictly
    h.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)


def test_head_optimizer_groups_follow_the_constructor_rule():
    """lr scale 1 (non-backbone names fall into the last layer of the reference's layer-decay constructors) and no weight decay for 1-D parameters
    and biases"""
    from mtp_amd.parallel import head_param_groups
    h = small_head(slice_classes=(4, 6, 8))
    names = h.trained_parameter_names()
    assert not any(n.startswith("conv_seg.") for n in names) and "semseghead_1.1.weight" in names
    shapes = {n: tuple(p.shape) for n, p in h.named_parameters()}
    groups = head_param_groups(names, shapes, 0.05)
    assert [(g, s, w) for g, s, w, _ in groups] == [("decode_head.decay", 1.0, 0.05), ("decode_head.no_decay", 1.0, 0.0)]
    dec, nd = groups[0][3], groups[1][3]
    assert sorted(dec + nd) == sorted(names)
    assert all(len(shapes[n]) == 4 for n in dec) and all(len(shapes[n]) == 1 or n.endswith(".bias") for n in nd)
    assert "bottleneck.bn.weight" in nd and "semseghead_2.1.bias" in nd and "fpn_convs.0.conv.weight" in dec
    assert small_head().trained_parameter_names()[:2] == ["conv_seg.weight", "conv_seg.bias"]
