"""CPU: the change-detection model's host side.
  * the torch restatement the GPU tests compare against (tests/unet_ref.py) equals the reference's own UNetHead, fixture f19, at 1e-5 for both
    geometries: training-mode logits, loss, d(inputs), every parameter gradient, the updated running statistics, eval-mode logits;
  * mtp_amd.UNetHead's ordered state-dict keys and shapes equal the reference head's recorded list; the registry builds the Levir config's model dict;
    what the constructor refuses;
  * FeatureFusionNeck's four policies and SiamEncoderDecoder's split against torch expressions, with torch stand-ins for the kernels (no GPU here)."""
import json
import os

import numpy as np
import pytest
import torch

import mtp_amd
import unet_ref as R
from mtp_amd import MODELS, FeatureFusionNeck, SiamEncoderDecoder, UNetHead, ops


def _head(tag, **kw):
    chans = R.F19_GEOMS[tag][0]
    return UNetHead(**dict(R.F19_HEAD, in_channels=chans, encoder_channels=chans, **kw))


# ------------------------------------------------------------------------------------------------ fixture f19: the reference's own UNetHead
@pytest.mark.parametrize("tag", sorted(R.F19_GEOMS))
def test_torch_restatement_pinned_to_f19(golden, tag):
    from conftest import rel_err
    d = golden("f19_unet.npz")
    sd, ins, lab, mask = R.f19_case(golden, tag)
    chans, sizes, lab_size = R.F19_GEOMS[tag]
    assert [tuple(x.shape[1:]) for x in ins] == [(c,) + s for c, s in zip(chans, sizes)] and tuple(lab.shape[1:]) == lab_size
    assert (lab == 255).any() and (mask == 0).any()
    for k in sd:
        sd[k].requires_grad_(sd[k].is_floating_point() and "running" not in k)
    xi = [x.clone().requires_grad_(True) for x in ins]
    logits = R.torch_unet(sd, xi, 4, True, mask)
    assert tuple(logits.shape[2:]) == ((64, 96) if tag == "flat" else (32, 64))       # flat: finer than the labels, the loss's resize shrinks them
    loss = R.torch_seg_loss(logits, lab)
    loss.backward()
    assert rel_err(logits.detach(), torch.from_numpy(d[tag + ".logits_train"])) < 1e-5
    assert abs(loss.item() - float(d[tag + ".loss"])) < 1e-5 * float(d[tag + ".loss"])
    for i, x in enumerate(xi):
        assert rel_err(x.grad, torch.from_numpy(d[tag + ".dinput%d" % i])) < 1e-5
    h = _head(tag)
    for n, _ in h.named_parameters():
        assert rel_err(sd[n].grad, torch.from_numpy(d[tag + ".grad." + n])) < 1e-5, n
    for n, _ in h.named_buffers():
        ref = torch.from_numpy(d[tag + ".after." + n])
        if ref.is_floating_point():
            assert rel_err(sd[n].detach(), ref) < 1e-5, n
        else:       # num_batches_tracked: one training forward (F.batch_norm itself does not count)
            assert int(ref) == int(sd[n]) + 1, n
    sde, ins_e, _, _ = R.f19_case(golden, tag)
    with torch.no_grad():
        ev = R.torch_unet(sde, ins_e, 4, False)
    assert rel_err(ev, torch.from_numpy(d[tag + ".logits_eval"])) < 1e-5
    # and the module loads the reference's state dict strictly
    h.load_state_dict({k: v.detach().float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)


def test_classifier_before_the_final_resize_equals_the_reference_order(golden):
    """the engine's order (Dropout2d -> 1x1 conv on the last block's grid, then the x2 bilinear resize of the logits) against the reference's
    (resize, Dropout2d, conv) in float64"""
    import torch.nn.functional as F
    sd, ins, _, mask = R.f19_case(golden, "pyr")
    with torch.no_grad():
        ref = R.torch_unet(sd, ins, 4, False, mask)
        feat = R.torch_unet_feature(sd, ins, 4, False)
        ours = F.interpolate(F.conv2d(feat * mask[:, :, None, None], sd["conv_seg.weight"], sd["conv_seg.bias"]), scale_factor=2, mode="bilinear")
    assert (ours - ref).abs().max().item() < 1e-12


# ------------------------------------------------------------------------------------------------ the module surface
def test_state_dict_keys_order_and_shapes_equal_the_reference_heads():
    from conftest import GOLDEN
    ref = json.loads(str(np.load(os.path.join(GOLDEN, "f19_unet.npz"))["levir_keys"]))
    h = MODELS.build(dict(R.LEVIR_HEAD))
    assert [[k, list(v.shape)] for k, v in h.state_dict().items()] == ref
    assert [(k, tuple(s)) for k, s in ref] == R.unet_keys([1024] * 4, [512, 256, 128, 64], 2)
    for tag, (chans, _, _) in R.F19_GEOMS.items():
        assert [(k, tuple(v.shape)) for k, v in _head(tag).state_dict().items()] == R.unet_keys(chans, R.F19_HEAD["decoder_channels"], 2)


def test_head_surface_and_init():
    h = MODELS.build(dict(R.LEVIR_HEAD))
    assert isinstance(h, UNetHead) and mtp_amd.UNetHead is UNetHead and h.sync_bn and h.in_index == [0, 1, 2, 3] and h.num_classes == 2 and h.channels == 64
    assert h.blocks[0].conv1[0].weight.shape == (512, 2048, 3, 3) and h.blocks[0].conv1[0].bias is None and h.blocks[3].conv1[0].weight.shape == (64, 128, 3, 3)
    assert abs(h.conv_seg.weight.std().item() - 0.01) < 0.004 and h.conv_seg.bias.abs().max() == 0
    assert h.trained_parameter_names() == [n for n, _ in h.named_parameters()]
    for name in ("forward", "_forward_feature", "cls_seg", "loss_by_feat", "loss", "predict", "loss_and_grads", "logit_rows"):
        assert callable(getattr(h, name))
    assert h.dropout_mask is None and not hasattr(h, "bn_reduce")


def test_registry_builds_the_levir_model_dict():
    """the config's model= dict with the backbone shrunk (the config's ViT-L is 300 M parameters); open-cd's body of `RVSA_MTP` (taps, frozen_stages) is
    registered here as RVSA_MTP_taps"""
    model = dict(type="SiamEncoderDecoder", data_preprocessor=None,
                 backbone=dict(type="RVSA_MTP_taps", img_size=64, patch_size=16, drop_path_rate=0.0, out_indices=[0, 1, 2, 3], embed_dim=128, depth=4, num_heads=2,
                               mlp_ratio=4, qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., use_checkpoint=False, use_abs_pos_emb=True,
                               interval=2, frozen_stages=-1),
                 neck=dict(R.LEVIR_NECK),
                 decode_head=dict(R.LEVIR_HEAD, in_channels=[128] * 4, encoder_channels=[128] * 4),
                 train_cfg=dict(), test_cfg=dict(mode="whole"))
    m = MODELS.build(model)
    assert isinstance(m, SiamEncoderDecoder) and isinstance(m.neck, FeatureFusionNeck) and isinstance(m.decode_head, UNetHead)
    assert m.neck.policy == "abs_diff" and m.neck.out_indices == (0, 1, 2, 3) and m.backbone_inchannels == 3 and m.num_classes == 2
    with pytest.raises(ValueError):
        MODELS.build(dict(model, neck=None))


@pytest.mark.parametrize("bad,exc", [(dict(center=True), NotImplementedError), (dict(attention_type="scse"), NotImplementedError),
                                     (dict(use_batchnorm=False), NotImplementedError), (dict(use_batchnorm="inplace"), NotImplementedError),
                                     (dict(align_corners=True), NotImplementedError), (dict(n_blocks=3), ValueError),
                                     (dict(decoder_channels=[32, 16, 8, 12], channels=12), NotImplementedError), (dict(channels=16), ValueError)])
def test_unsupported_configurations_raise(bad, exc):
    with pytest.raises(exc):
        _head("flat", **bad)


# ------------------------------------------------------------------------------------------------ neck and siamese split (torch stand-ins for the kernels)
def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


@pytest.fixture
def standins(monkeypatch):
    """torch expressions in place of the four kernels the neck calls -- the host logic around them (halves, policies, level selection, autograd
    wiring, dtypes) is what runs here; the kernels themselves are held to the same expressions bit for bit in test_hip_unet_head.py"""
    def fuse_fwd(f, out, policy):
        N = f.shape[0] // 2
        out.copy_(_rows(R.torch_fuse(f[:N].float(), f[N:].float(), policy)))
        return out

    def fuse_bwd(g, f, df, policy):
        N, C, H, W = df.shape[0] // 2, df.shape[1], df.shape[2], df.shape[3]
        with torch.enable_grad():        # (called from inside a backward pass)
            x = f.detach().float().requires_grad_(True)
            y = _rows(R.torch_fuse(x[:N], x[N:], policy))
            df.copy_(torch.autograd.grad(y, x, g)[0])
        return df

    def t2n(x, out, B, H, W, levels):
        out.copy_(x.reshape(B, H, W, -1).permute(0, 3, 1, 2))
        return out

    def n2t(f, out, B, H, W, levels):
        out.copy_(_rows(f))
        return out
    for name, fn in (("fuse_pair_fwd", fuse_fwd), ("fuse_pair_bwd", fuse_bwd), ("tokens_to_nchw", t2n), ("nchw_to_tokens", n2t)):
        monkeypatch.setattr(ops, name, fn)


@pytest.mark.parametrize("policy", ["concat", "sum", "diff", "abs_diff"])
def test_neck_policies_against_torch(standins, policy):
    g = torch.Generator().manual_seed(1)
    x1 = [torch.randn(2, c, s, s + 1, generator=g) for c, s in ((8, 4), (16, 3), (8, 2), (24, 1))]
    x2 = [torch.randn(t.shape, generator=g) for t in x1]
    x2[0][:, :, 0] = x1[0][:, :, 0]          # equal pixels: abs_diff's gradient is 0 there, on both sides
    neck = MODELS.build(dict(type="FeatureFusionNeck", policy=policy, out_indices=(0, 2, 3)))
    a = [t.clone().requires_grad_(True) for t in x1 + x2]
    b = [t.clone().requires_grad_(True) for t in x1 + x2]
    outs, refs = neck(a[:4], a[4:]), R.torch_neck(b[:4], b[4:], policy, (0, 2, 3))
    assert len(outs) == 3
    w = [torch.randn(r.shape, generator=g) for r in refs]
    sum((o * v).sum() for o, v in zip(outs, w)).backward()
    sum((o * v).sum() for o, v in zip(refs, w)).backward()
    for o, r in zip(outs, refs):
        assert o.shape == r.shape and torch.equal(o, r)
    for i, (p, q) in enumerate(zip(a, b)):
        if i % 4 == 1:
            assert p.grad is None and q.grad is None       # level 1 is not in out_indices
        else:
            assert torch.equal(p.grad, q.grad)
    # the 2N-batch form the segmentor uses
    for o, r in zip(neck.forward_batch([torch.cat([u, v]) for u, v in zip(x1, x2)]), refs):
        assert torch.equal(o, r)


def test_neck_refuses_unknown_policy_and_mismatched_inputs(standins):
    with pytest.raises(ValueError):
        FeatureFusionNeck(policy="max")
    with pytest.raises(ValueError):
        ops.fuse_policy("abs-diff")
    n = FeatureFusionNeck(policy="sum")
    with pytest.raises(ValueError):
        n([torch.zeros(1, 8, 2, 2)], [torch.zeros(1, 8, 2, 3)])
    with pytest.raises(ValueError):
        n([torch.zeros(1, 8, 2, 2)] * 2, [torch.zeros(1, 8, 2, 2)])


class _Taps(torch.nn.Module):
    """a stand-in backbone: four per-sample maps that tell the samples and channels apart"""

    def forward(self, x):
        self.seen = x
        return tuple(torch.cat([x[:, :, ::s, ::s]] * 8, 1)[:, :8] * (i + 1) for i, s in enumerate((4, 8, 16, 16)))


def test_siamese_split_and_extract_feat_against_torch(standins):
    g = torch.Generator().manual_seed(2)
    head = UNetHead(encoder_channels=[8] * 4, decoder_channels=[8] * 4, n_blocks=4, num_classes=2)
    m = SiamEncoderDecoder(_Taps(), head, neck=dict(type="FeatureFusionNeck", policy="abs_diff"), test_cfg=dict(mode="whole"))
    x = torch.randn(3, 6, 32, 32, generator=g)
    a, b = R.torch_siam_split(x, 3)
    assert torch.equal(m.split(x), torch.cat([a, b]))
    feats = m.extract_feat(x)
    assert torch.equal(m.backbone.seen, torch.cat([a, b]))             # one backbone pass on the 2N-batch, "from" images first
    bb = _Taps()
    for f, r in zip(feats, R.torch_neck(bb(a), bb(b), "abs_diff")):
        assert f.shape[0] == 3 and torch.equal(f, r)
    with pytest.raises(ValueError):
        m.split(torch.zeros(1, 3, 32, 32))
    assert SiamEncoderDecoder(_Taps(), head, neck=m.neck, test_cfg=dict(mode="slide", crop_size=(16, 16), stride=(8, 8))).test_cfg["mode"] == "slide"
