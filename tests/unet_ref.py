"""The torch restatement of the change-detection model that the tests share: the reference's UNetHead forward (RS_Tasks_Finetune/Change_Detection/
opencd/models/decode_heads/unet_head.py) + BaseDecodeHead's loss on a state dict, pinned to the reference's own code by fixture f19
(test_unet_head.py); open-cd's FeatureFusionNeck policies and SiamEncoderDecoder split as torch expressions.  Plain helper module, no tests."""
import torch
import torch.nn.functional as F

# probe: when a list, every Conv2dReLU appends min |pre-activation| -- how close the batch comes to the ReLU's kink
probe = None

# RS_Tasks_Finetune/Change_Detection/configs/mtp/levir/rvsa-l-unet-256-mae-mtp_levir.py, model.decode_head / model.neck
LEVIR_HEAD = dict(type="UNetHead", num_classes=2, ignore_index=255, in_channels=[1024, 1024, 1024, 1024], in_index=[0, 1, 2, 3], channels=64,
                  dropout_ratio=0.1, encoder_channels=[1024, 1024, 1024, 1024], decoder_channels=[512, 256, 128, 64], n_blocks=4, use_batchnorm=True,
                  center=False, attention_type=None, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
                  loss_decode=dict(type="mmseg.CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0))
LEVIR_NECK = dict(type="FeatureFusionNeck", policy="abs_diff", out_indices=(0, 1, 2, 3))

# fixture f19's reduced head and its two geometries: (channels, (H, W)) per level, and the label size
F19_HEAD = dict(num_classes=2, channels=8, dropout_ratio=0.1, decoder_channels=[32, 16, 8, 8], n_blocks=4)
F19_GEOMS = {"flat": ([16, 16, 16, 16], [(2, 3)] * 4, (32, 48)), "pyr": ([8, 16, 24, 32], [(8, 12), (4, 6), (2, 3), (1, 2)], (32, 64))}


def unet_keys(encoder_channels, decoder_channels, num_classes):
    """the reference UNetHead's state-dict order: BaseDecodeHead's conv_seg, then per block conv1 / conv2 = Sequential(conv, norm, relu)"""
    rev = list(encoder_channels)[::-1]
    cin = [rev[0]] + list(decoder_channels[:-1])
    cskip = (rev[1:] + [0] * len(decoder_channels))[:len(decoder_channels)]
    keys = [("conv_seg.weight", (num_classes, decoder_channels[-1], 1, 1)), ("conv_seg.bias", (num_classes,))]
    for i, (a, s, o) in enumerate(zip(cin, cskip, decoder_channels)):
        for name, ci in (("conv1", a + s), ("conv2", o)):
            pre = "blocks.%d.%s" % (i, name)
            keys += [(pre + ".0.weight", (o, ci, 3, 3))] + [(pre + ".1." + n, (o,)) for n in ("weight", "bias", "running_mean", "running_var")]
            keys += [(pre + ".1.num_batches_tracked", ())]
    return keys


def _cbr(sd, pre, x, training):
    x = F.conv2d(x, sd[pre + ".0.weight"], None, padding=1)
    x = F.batch_norm(x, sd[pre + ".1.running_mean"], sd[pre + ".1.running_var"], sd[pre + ".1.weight"], sd[pre + ".1.bias"], training, 0.1, 1e-5)
    if probe is not None:
        probe.append(x.detach().abs().min().item())
    return F.relu(x)


def torch_unet_feature(sd, inputs, n_blocks, training):
    """UNetHead.forward up to the last DecoderBlock (running statistics updated in place in training mode)"""
    feats = list(inputs)[::-1]
    x, skips = feats[0], feats[1:]
    for i in range(n_blocks):
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        if i < len(skips):
            x = torch.cat([x, F.interpolate(skips[i], size=x.shape[2:], mode="bilinear")], 1)
        x = _cbr(sd, "blocks.%d.conv2" % i, _cbr(sd, "blocks.%d.conv1" % i, x, training), training)
    return x


def torch_unet(sd, inputs, n_blocks, training, mask=None):
    """the whole forward: the blocks, F.interpolate(x2, bilinear), cls_seg with Dropout2d as an explicit (N, C) mask of 0 and 1 / (1 - p)"""
    x = F.interpolate(torch_unet_feature(sd, inputs, n_blocks, training), scale_factor=2, mode="bilinear")
    if mask is not None:
        x = x * mask[:, :, None, None]
    return F.conv2d(x, sd["conv_seg.weight"], sd["conv_seg.bias"])


def torch_seg_loss(logits, labels, ignore_index=255, loss_weight=1.0):
    """BaseDecodeHead.loss_by_feat: resize the logits to the labels, CrossEntropyLoss(avg_non_ignore=False) = sum over kept pixels / all pixels"""
    up = F.interpolate(logits, size=labels.shape[1:], mode="bilinear", align_corners=False)
    return loss_weight * F.cross_entropy(up, labels.long(), ignore_index=ignore_index, reduction="sum") / labels.numel()


def torch_fuse(x1, x2, policy):
    """open-cd FeatureFusionNeck.fusion"""
    if policy == "concat":
        return torch.cat([x1, x2], 1)
    if policy == "sum":
        return x1 + x2
    if policy == "diff":
        return x2 - x1
    if policy == "abs_diff":
        return (x1 - x2).abs()
    raise ValueError(policy)


def torch_neck(x1, x2, policy, out_indices=(0, 1, 2, 3)):
    outs = [torch_fuse(a, b, policy) for a, b in zip(x1, x2)]
    return tuple(outs[i] for i in out_indices)


def torch_siam_split(inputs, c=3):
    """open-cd SiamEncoderDecoder.extract_feat's split of the (N, 2c, H, W) input"""
    return torch.split(inputs, c, dim=1)


def f19_case(golden, tag, dtype=torch.float64):
    """(state dict, inputs, labels, dropout mask) of fixture f19's geometry `tag` ('flat' / 'pyr')"""
    d = golden("f19_unet.npz")
    pre = tag + ".init."
    sd = {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in d.items() if k.startswith(pre)}
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    ins = [torch.from_numpy(d[tag + ".input%d" % i]).to(dtype) for i in range(4)]
    return sd, ins, torch.from_numpy(d[tag + ".labels"]), torch.from_numpy(d[tag + ".mask"]).to(dtype)
