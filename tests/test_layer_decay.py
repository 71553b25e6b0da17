"""CPU: layer-wise lr decay -- the parameter groups of the reference's two layer-decay constructors (fixture f16, generated from
mmcv_custom/layer_decay_optimizer_constructor_vit.py and custom_layer_decay_optimizer_constructor.py by make_param_groups.py), the flat
optimizer's per-segment tables built from them, and checkpoint / scheduler parity with a torch.optim.AdamW built from the same groups."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import mtp_amd
from conftest import GOLDEN
from mtp_amd.optim_groups import PRETRAIN_OPTIM_WRAPPERS, layer_decay_param_groups, pretrain_optim_wrapper
from mtp_amd.parallel import DataParallelTrainer, FlatAdamW, FlatParams, reference_param_groups


@pytest.fixture(scope="module")
def f16():
    d = np.load(os.path.join(GOLDEN, "f16_param_groups.npz"))
    return json.loads(str(d["cases"])), d


MODELS = {
    "vit_b": lambda: mtp_amd.vit_b_rvsa(type("A", (), dict(image_size=224, use_ckpt="False"))),
    "vit_l": lambda: mtp_amd.vit_l_rvsa(type("A", (), dict(image_size=224, use_ckpt="False"))),
    "internimage_xl": lambda: mtp_amd.internimage_xl(),
    "internimage_l2postnorm": lambda: mtp_amd.InternImage(channels=32, depths=[5, 5, 24, 5], groups=[2, 4, 8, 16], layer_scale=None, post_norm=False,
                                                          res_post_norm=True, level2_post_norm=True, level2_post_norm_block_ids=[5, 11, 17, 23],
                                                          dw_kernel_size=5, center_feature_scale=True, drop_path_rate=0.0),
}


@pytest.mark.parametrize("model", sorted(MODELS))
def test_builder_reproduces_the_reference_groups(f16, model):
    """the repo module has the reference backbone's (name, shape) list, and the builder gives every parameter the group -- name, lr scale to 1e-12,
    weight decay, first-seen order -- that the reference's constructor gave it, under each prefix the fixture records"""
    cases, d = f16
    named = [(n, tuple(p.shape)) for n, p in MODELS[model]().named_parameters()]
    assert hashlib.sha256("\n".join("%s %s" % (n, list(s)) for n, s in named).encode()).hexdigest() == str(d[model + ".names_digest"])
    tags = [t for t, c in cases.items() if c["model"] == model]
    assert tags
    for tag in tags:
        got = layer_decay_param_groups(named, cases[tag]["optim_wrapper"], prefix=cases[tag]["prefix"])
        gid = d[tag + ".gid"]
        assert [g[0] for g in got] == d[tag + ".group_names"].tolist(), tag
        for k, (gn, scale, wd, names) in enumerate(got):
            assert names == [named[i][0] for i in np.flatnonzero(gid == k)], (tag, gn)
            ws = float(d[tag + ".scales"][k])
            assert wd == float(d[tag + ".wds"][k]) and abs(scale - ws) <= 1e-12 * ws, (tag, gn, scale, ws)
    if model == "vit_l":      # the fine-tune prefix gives ViT-L 52 groups from 0.9 ** 25; the pretraining prefix makes the rule a no-op
        assert len(d["vit_l_backbone.scales"]) == 52 and d["vit_l_backbone.scales"].min() == pytest.approx(0.9 ** 25)
        assert d["vit_l_encoder.scales"].tolist() == [1.0, 1.0]


def test_presets_are_the_reference_pretraining_optimizers():
    # main_pretrain.py:429-451 (ViT-B / ViT-L) and :464-472 (InternImage-XL)
    for k, layers in (("vit_b", 12), ("vit_l", 24)):
        ow = pretrain_optim_wrapper(k)
        assert ow["optimizer"] == dict(type="AdamW", lr=6e-5, betas=(0.9, 0.999), weight_decay=0.05)
        assert ow["constructor"] == "LayerDecayOptimizerConstructor_ViT" and ow["paramwise_cfg"] == dict(num_layers=layers, layer_decay_rate=0.9)
    ow = pretrain_optim_wrapper("internimage_xl")
    assert ow["optimizer"] == dict(type="AdamW", lr=2e-5, betas=(0.9, 0.999), weight_decay=0.05)
    assert ow["constructor"] == "CustomLayerDecayOptimizerConstructor_InternImage"
    assert ow["paramwise_cfg"] == dict(num_layers=39, layer_decay_rate=0.94, depths=[5, 5, 24, 5])
    ow["paramwise_cfg"]["num_layers"] = 1
    assert PRETRAIN_OPTIM_WRAPPERS["internimage_xl"]["paramwise_cfg"]["num_layers"] == 39        # a copy
    with pytest.raises(KeyError):
        pretrain_optim_wrapper("vit_h")


def small_vit():
    torch.manual_seed(0)
    return mtp_amd.ViT_Win_RVSA_V3_WSZ7(embed_dim=128, depth=6, num_heads=2, interval=3, qkv_bias=True, use_abs_pos_emb=True, out_indices=[1, 2, 3, 5])


def small_wrapper(depth=6):
    ow = pretrain_optim_wrapper("vit_b")
    ow["paramwise_cfg"]["num_layers"] = depth
    return ow


def test_segment_tables_give_every_parameter_its_group():
    net = small_vit()
    groups = layer_decay_param_groups(net.named_parameters(), small_wrapper(), prefix="backbone.")
    assert len(groups) == 2 * (6 + 2) and groups[0][0] == "layer_0_no_decay"        # (decay + no_decay for layer 0, the six blocks and the rest)
    flat = FlatParams(net, unused=net._unused_params)
    opt = FlatAdamW(flat, param_groups=groups)
    of = {n: (s, wd) for _, s, wd, ns in groups for n in ns}
    st, wd, lr = opt.seg_start.tolist(), opt.seg_wd.tolist(), opt.seg_lr.tolist()
    assert st == [flat.offsets[n] for n in flat.names]
    for n, w, s in zip(flat.names, wd, lr):
        assert w == pytest.approx(of[n][1]) and s == pytest.approx(of[n][0], rel=1e-7), n
    assert lr[flat.names.index("blocks.0.attn.qkv.weight")] == pytest.approx(0.9 ** 6)
    assert lr[flat.names.index("patch_embed.proj.weight")] == pytest.approx(0.9 ** 7)
    assert lr[flat.names.index("fpn1.0.weight")] == 1.0
    # without groups: the tables of before, no scale table
    plain = FlatAdamW(FlatParams(small_vit(), unused=net._unused_params))
    assert plain.seg_lr is None and plain.param_groups is None
    st0, wd0 = flat.weight_decay_segments(0.05)
    assert torch.equal(plain.seg_start, st0) and torch.equal(plain.seg_wd, wd0)
    # a parameter in no group
    with pytest.raises(ValueError, match="no optimizer group"):
        FlatAdamW(FlatParams(small_vit(), unused=net._unused_params), param_groups=[(g, s, w, [n for n in ns if n != "blocks.1.mlp.fc1.weight"]) for g, s, w, ns in groups])


def _torch_adamw(net, groups, lr, wd):
    P = dict(net.named_parameters())
    return torch.optim.AdamW([{"params": [P[n] for n in names], "weight_decay": gwd, "lr": lr * scale, "param_names": list(names), "lr_scale": scale,
                               "group_name": g} for g, scale, gwd, names in groups], lr=lr, betas=(0.9, 0.999), weight_decay=wd)


@pytest.mark.parametrize("kind", ["vit", "internimage"])
def test_state_dict_round_trips_through_torch_adamw_with_the_same_groups(kind):
    if kind == "vit":
        net, ow, prefix = small_vit(), small_wrapper(), "backbone."
    else:
        import recipe
        c = recipe.II_CFG
        torch.manual_seed(0)
        net = mtp_amd.InternImage(channels=c["channels"], depths=c["depths"], groups=c["groups"], layer_scale=c["layer_scale"], offset_scale=c["offset_scale"],
                                  post_norm=True, drop_path_rate=0.0)
        ow, prefix = pretrain_optim_wrapper("internimage_xl"), "encoder."
        ow["paramwise_cfg"].update(num_layers=sum(c["depths"]), depths=c["depths"])
    lr0 = ow["optimizer"]["lr"]
    groups = layer_decay_param_groups(net.named_parameters(), ow, prefix=prefix)
    assert len(set(s for _, s, _, _ in groups)) > 3
    flat = FlatParams(net, unused=net._unused_params)
    opt = FlatAdamW(flat, lr=lr0, total_steps=100, param_groups=groups)
    g = torch.Generator().manual_seed(1)
    opt.m.copy_(torch.randn(opt.m.shape, generator=g))
    opt.v.copy_(torch.rand(opt.v.shape, generator=g))
    opt.t = opt.last_epoch = 7
    sd = opt.state_dict(net)
    ref = _torch_adamw(net, groups, lr0, 0.05)
    ref.load_state_dict(sd)
    assert len(ref.param_groups) == len(groups)
    for pg, (gn, scale, wd, names) in zip(ref.param_groups, groups):
        assert pg["group_name"] == gn and pg["lr_scale"] == scale and pg["weight_decay"] == wd and pg["param_names"] == names
        assert pg["lr"] == pytest.approx(opt.lr_at(7) * scale) and pg["initial_lr"] == pytest.approx(lr0 * scale)
    P = dict(net.named_parameters())
    for n in flat.names:
        if flat.groups[n] is None:
            assert P[n] not in ref.state
            continue
        st = ref.state[P[n]]
        assert torch.equal(st["exp_avg"], flat.view(opt.m, n)) and torch.equal(st["exp_avg_sq"], flat.view(opt.v, n)) and float(st["step"]) == 7
    # torch's state dict back into a fresh flat optimizer built from the same groups
    opt2 = FlatAdamW(FlatParams(net, unused=net._unused_params), lr=lr0, total_steps=100, param_groups=groups)
    assert opt2.load_state_dict(ref.state_dict(), net) == sum(1 for n in flat.names if flat.groups[n] is not None)
    used = torch.zeros_like(opt.m, dtype=torch.bool)
    for n in flat.names:
        if flat.groups[n] is not None:
            flat.view(used, n).fill_(True)
    assert opt2.t == 7 and torch.equal(opt2.m[used], opt.m[used]) and torch.equal(opt2.v[used], opt.v[used])
    # the scheduler: one base lr per group
    ssd = opt.scheduler_state_dict()
    assert ssd["base_lrs"] == pytest.approx([lr0 * s for _, s, _, _ in groups]) and len(ssd["_last_lr"]) == len(groups)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ref, 100, eta_min=0, last_epoch=-1)
    sched.load_state_dict(ssd)
    assert sched.last_epoch == 7 and sched.get_last_lr() == pytest.approx([opt.lr_at(7) * s for _, s, _, _ in groups])
    sched.step()
    assert [pg["lr"] for pg in ref.param_groups] == pytest.approx([opt.lr_at(8) * s for _, s, _, _ in groups], rel=1e-9)


def test_trainer_takes_the_reference_optim_wrapper():
    net = small_vit()
    ow = small_wrapper()
    ow["optimizer"].update(lr=3e-4, betas=(0.8, 0.99), weight_decay=0.1)
    tr = DataParallelTrainer(net, lr=1.0, weight_decay=0.5, total_steps=10, optim_wrapper=ow, param_prefix="backbone.")
    assert tr.opt.lr0 == 3e-4 and tr.opt.betas == (0.8, 0.99) and tr.opt.weight_decay == 0.1
    assert tr.opt.param_groups == layer_decay_param_groups(net.named_parameters(), ow, prefix="backbone.")
    sd = tr.checkpoint()["optimizer"]
    assert len(sd["param_groups"]) == 16 and {pg["weight_decay"] for pg in sd["param_groups"]} == {0.0, 0.1}
    # the pretraining prefix: the ViT rule is a no-op -- the same two groups as reference_param_groups, scale 1
    tr2 = DataParallelTrainer(small_vit(), total_steps=10, optim_wrapper=small_wrapper())
    assert [(g, s, w, n) for g, s, w, n in tr2.opt.param_groups] == reference_param_groups(tr2.module.named_parameters(), 0.05)
    # no optim_wrapper: nothing changes
    tr3 = DataParallelTrainer(small_vit(), total_steps=10)
    assert tr3.opt.param_groups is None and tr3.opt.seg_lr is None and tr3.opt.scheduler_state_dict()["base_lrs"] == [6e-5, 6e-5]


def test_frozen_parameters_are_refused_with_layer_decay():
    net = small_vit()
    net.blocks[2].attn.qkv.weight.requires_grad_(False)
    with pytest.raises(ValueError, match="requires_grad=False"):
        DataParallelTrainer(net, total_steps=10, optim_wrapper=small_wrapper(), param_prefix="backbone.")
