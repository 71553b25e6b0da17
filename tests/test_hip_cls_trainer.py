"""GPU: LinearClsHead trained together with the backbone by DataParallelTrainer(decode_head=...) -- one clip norm over backbone and head, AdamW with
the reference's groups on both -- against torch: autograd through the project's CPU restatement of the backbone (oracle/) and torch operators for the
neck, the head and the loss, torch.nn.utils.clip_grad_norm_ over both parameter lists, torch.optim.AdamW.  Built as tests/test_hip_uper_trainer.py
builds it, with that file's bounds.  Also the checkpoint round trip with the head attached, and one step over the smallest InternImage configuration
tests/test_hip_internimage.py trains, head on its last map, against oracle.internimage_oracle at that file's fp32 gradient bound (1e-3)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import mtp_amd
from conftest import ROOT, rel_err
from mtp_amd import LinearClsHead
from oracle import internimage_oracle as IO
from oracle import vit_rvsa_oracle as O

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import recipe  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = dict(embed_dim=128, depth=4, heads=2, interval=3)
LR, WD, MAX_NORM = 1e-3, 0.05, 0.01
K = 7


def _net(params):
    net = mtp_amd.RVSA_MTP_taps(img_size=224, embed_dim=128, depth=4, num_heads=2, interval=3, qkv_bias=True, use_abs_pos_emb=True, out_indices=[1, 3],
                                drop_path_rate=0.0, precision="fp32", feature_dtype=torch.float32)
    net.load_state_dict(params, strict=False)
    return net.cuda().train()


def _head(seed, in_channels=128):
    g = torch.Generator().manual_seed(seed)
    head = LinearClsHead(K, in_channels, topk=(1, 5))
    with torch.no_grad():      # N(0, 1): the default N(0, 0.01) leaves gradients of rounding size in the backbone
        head.fc.weight.copy_(torch.randn(K, in_channels, generator=g))
        head.fc.bias.copy_(torch.randn(K, generator=g))
    return head


def _setup(seed=0):
    params = recipe.make_params(recipe.state_shapes(CFG["embed_dim"], CFG["depth"], CFG["heads"], CFG["interval"]))
    img = recipe.make_input(2, 224, 224, seed=7)
    lab = torch.tensor([[6, 0], [3, 3]])
    return params, _head(seed), img, lab


def _torch_loss(feats, hd, labels):
    return F.cross_entropy(F.linear(F.adaptive_avg_pool2d(feats[-1], 1).flatten(1), hd["fc.weight"], hd["fc.bias"]), labels)


def test_trainer_step_with_cls_head_matches_torch_autograd_clip_and_adamw():
    from mtp_amd.parallel import DataParallelTrainer, head_param_groups, reference_param_groups
    params, head, img, lab = _setup()
    sd0 = {k: v.clone() for k, v in head.state_dict().items()}
    net = _net(params)
    tr = DataParallelTrainer(net, lr=LR, weight_decay=WD, max_norm=MAX_NORM, feature_dtype=torch.float32, decode_head=head.cuda().train())
    bb = {n: params[n].clone().requires_grad_(True) for n, _ in net.named_parameters() if n in tr.flat.offsets and tr.flat.groups[n] is not None}
    fixed = {n: v for n, v in params.items() if n not in bb}
    hd = {k: v.clone().float().requires_grad_(True) for k, v in sd0.items()}
    hnames = tr.hflat.names
    assert hnames == ["fc.weight", "fc.bias"]
    shapes = {n: tuple(hd[n].shape) for n in hnames}
    groups = [(g, s, w, [bb[n] for n in ns if n in bb]) for g, s, w, ns in reference_param_groups(net.named_parameters(), WD)] + \
             [(g, s, w, [hd[n] for n in ns]) for g, s, w, ns in head_param_groups(hnames, shapes, WD)]
    topt = torch.optim.AdamW([{"params": ps, "weight_decay": w} for _, _, w, ps in groups if ps], lr=LR, betas=(0.9, 0.999), eps=1e-8)
    for step in range(2):
        loss = tr.step(img.cuda(), head.loss_and_grads(lab[step].cuda()))
        torch.cuda.synchronize()
        if step == 0:
            g_bb = {n: tr.flat.view(tr.flat.grad, n).cpu().clone() for n in bb}
            g_hd = {n: tr.hflat.view(tr.hflat.grad, n).cpu().clone() for n in hnames}
            sqn = float(tr.opt.sqn.item())
        feats = O.backbone_forward(img, {**fixed, **bb}, CFG["depth"], CFG["heads"], CFG["interval"], [1, 3], taps_only=True)
        ref_loss = _torch_loss(feats, hd, lab[step])
        topt.zero_grad()
        ref_loss.backward()
        assert abs(loss.item() - ref_loss.item()) < 1e-3 * ref_loss.item()
        live = [p for p in list(bb.values()) + [hd[n] for n in hnames] if p.grad is not None]
        if step == 0:
            gmax = max(float(bb[n].grad.abs().max()) for n in bb if bb[n].grad is not None)
            for n in bb:
                if bb[n].grad is not None:
                    scale = max(float(bb[n].grad.abs().max()), 1e-2 * gmax)
                    assert float((g_bb[n] - bb[n].grad).abs().max()) < 2e-3 * scale, n
            for n in hnames:
                assert rel_err(g_hd[n], hd[n].grad) < 1e-3, n
            total = torch.nn.utils.clip_grad_norm_(live, MAX_NORM)
            assert total.item() > MAX_NORM        # (clipping active: the joint norm decides the step)
            assert abs(sqn ** 0.5 - total.item()) < 1e-3 * total.item()
        else:
            torch.nn.utils.clip_grad_norm_(live, MAX_NORM)
        topt.step()
    # parameters after two steps: Adam normalises, so an element whose gradient is within rounding of 0 may move by up to 2 lr either way; every
    # other element must agree
    gmax = max(float(bb[n].grad.abs().max()) for n in bb if bb[n].grad is not None)
    for n in hnames + list(bb):
        ours = dict(head.named_parameters())[n].detach().cpu() if n in hd else tr.flat.view(tr.flat.data, n).cpu()
        ref = (hd[n] if n in hd else bb[n]).detach()
        g = (hd[n] if n in hd else bb[n]).grad
        if g is None:
            continue
        if n in bb and float(g.abs().max()) < 1e-2 * gmax:
            assert float((ours - ref).abs().max()) <= 2 * 2 * LR + 1e-5, n
            continue
        bad = (ours - ref).abs() > 1e-5 + 1e-3 * LR
        tiny = g.abs() < 5e-3 * g.abs().max()
        assert bool((bad & ~tiny).sum() == 0), "%s: %d elements differ" % (n, int((bad & ~tiny).sum()))


def test_checkpoint_round_trip_with_cls_head():
    from mtp_amd.parallel import DataParallelTrainer
    params, head, img, lab = _setup(3)
    tr = DataParallelTrainer(_net(params), lr=LR, max_norm=MAX_NORM, feature_dtype=torch.float32, decode_head=head.cuda().train())
    tr.step(img.cuda(), head.loss_and_grads(lab[0].cuda()))
    ck = tr.checkpoint()
    dh = ck["decode_head"]
    assert list(dh["state_dict"]) == ["fc.weight", "fc.bias"] and dh["optimizer"]["names"] == ["fc.weight", "fc.bias"] and dh["optimizer"]["step"] == 1
    assert set(dh["optimizer"]["exp_avg"]) == set(dh["optimizer"]["exp_avg_sq"]) == {"fc.weight", "fc.bias"}
    assert float(dh["optimizer"]["exp_avg"]["fc.weight"].abs().max()) > 0
    head2 = _head(9)          # another initial state, overwritten by the load
    tr2 = DataParallelTrainer(_net(params), lr=LR, max_norm=MAX_NORM, feature_dtype=torch.float32, decode_head=head2.cuda().train())
    tr2.load_checkpoint(ck)
    for k, v in head.state_dict().items():
        assert torch.equal(v, head2.state_dict()[k]), k
    assert torch.equal(tr.hopt.m, tr2.hopt.m) and torch.equal(tr.hopt.v, tr2.hopt.v) and tr2.hopt.t == tr.hopt.t == 1
    assert torch.equal(tr.hflat.data, tr2.hflat.data)
    for t in (tr, tr2):
        t.module.train()
    tr.step(img.cuda(), head.loss_and_grads(lab[1].cuda()))
    tr2.step(img.cuda(), head2.loss_and_grads(lab[1].cuda()))
    torch.cuda.synchronize()
    assert rel_err(tr2.hflat.data.cpu(), tr.hflat.data.cpu()) < 1e-5 and rel_err(tr2.flat.data.cpu(), tr.flat.data.cpu()) < 1e-5


def test_internimage_step_with_cls_head_vs_oracle():
    from mtp_amd.parallel import DataParallelTrainer
    cfg = recipe.II_CFG
    net = mtp_amd.InternImage(core_op="DCNv3", channels=cfg["channels"], depths=cfg["depths"], groups=cfg["groups"], mlp_ratio=4.0, drop_path_rate=0.0,
                              norm_layer="LN", layer_scale=cfg["layer_scale"], offset_scale=cfg["offset_scale"], post_norm=True, with_cp=False,
                              out_indices=(0, 1, 2, 3), precision="fp32", feature_dtype=torch.float32)
    params = recipe.internimage_params(IO.state_shapes(cfg["channels"], cfg["depths"], cfg["groups"]))
    net.load_state_dict(params, strict=True)
    net = net.cuda().train()
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    labels = torch.tensor([6, 0])
    head = _head(4, in_channels=8 * cfg["channels"])
    hd = {k: v.clone().requires_grad_(True) for k, v in head.state_dict().items()}
    tr = DataParallelTrainer(net, lr=1e-3, weight_decay=0.05, max_norm=5.0, total_steps=10, feature_dtype=torch.float32, decode_head=head.cuda().train())
    loss = tr.step(img.cuda(), head.loss_and_grads(labels.cuda()))
    torch.cuda.synchronize()
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    feats = IO.backbone_forward(img, p, cfg["depths"], cfg["groups"], cfg["offset_scale"])
    assert tuple(feats[-1].shape) == (2, 8 * cfg["channels"], 2, 2)
    ref = _torch_loss(feats, hd, labels)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-3 * ref.item()
    for n in ("fc.weight", "fc.bias"):
        assert rel_err(tr.hflat.G[n].cpu(), hd[n].grad) < 1e-3, n
    for n, q in p.items():
        if q.grad is not None and n in tr.flat.G:
            assert rel_err(tr.flat.G[n].cpu(), q.grad) < 1e-3, n
