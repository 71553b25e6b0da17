"""GPU: the UperNet head trained together with the backbone by DataParallelTrainer(decode_head=...) -- one clip norm over encoder and decoder, AdamW with
the reference's groups on both, against torch: autograd through the project's CPU restatement of the backbone (oracle/) and the torch restatement of the
head, torch.nn.utils.clip_grad_norm_ over both parameter lists, torch.optim.AdamW.  Also the checkpoint round trip with the head attached, and a step
without a head."""
import os
import sys

import pytest
import torch

import mtp_amd
from conftest import ROOT, rel_err
from oracle import vit_rvsa_oracle as O
from test_uper_head import randomise_bn, small_head, torch_seg_loss, torch_uper

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import recipe  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = dict(embed_dim=128, depth=4, heads=2, interval=3)
LR, WD, MAX_NORM = 1e-3, 0.05, 0.01


def _net(params):
    net = mtp_amd.ViT_Win_RVSA_V3_WSZ7(img_size=224, embed_dim=128, depth=4, num_heads=2, interval=3, qkv_bias=True, use_abs_pos_emb=True,
                                       out_indices=[0, 1, 2, 3], drop_path_rate=0.0, precision="fp32", feature_dtype=torch.float32)
    net.load_state_dict(params, strict=False)
    return net.cuda().train()


def _setup(seed=0):
    params = recipe.make_params(recipe.state_shapes(CFG["embed_dim"], CFG["depth"], CFG["heads"], CFG["interval"]))
    head = randomise_bn(small_head(seed, in_channels=[128] * 4, channels=16, num_classes=5), seed + 1)
    g = torch.Generator().manual_seed(seed + 5)
    img = recipe.make_input(4, 224, 224, seed=7)
    lab = torch.randint(0, 5, (2, 4, 224, 224), generator=g)
    lab[torch.rand(lab.shape, generator=g) < 0.1] = 255
    masks = [(torch.rand(4, 16, generator=g) >= 0.1).float() / 0.9 for _ in range(2)]
    return params, head, img, lab, masks


def test_trainer_step_with_head_matches_torch_autograd_clip_and_adamw():
    from mtp_amd.parallel import DataParallelTrainer, head_param_groups, reference_param_groups
    params, head, img, lab, masks = _setup()
    sd0 = {k: v.clone() for k, v in head.state_dict().items()}
    net = _net(params)
    tr = DataParallelTrainer(net, lr=LR, weight_decay=WD, max_norm=MAX_NORM, feature_dtype=torch.float32, decode_head=head.cuda().train())
    # torch: the same parameters, autograd, one clip_grad_norm_ over both lists, AdamW with the reference's groups
    bb = {n: params[n].clone().requires_grad_(True) for n, _ in net.named_parameters() if n in tr.flat.offsets and tr.flat.groups[n] is not None}
    fixed = {n: v for n, v in params.items() if n not in bb}
    hd = {k: (v.clone().float().requires_grad_("running" not in k) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    hnames = tr.hflat.names
    shapes = {n: tuple(hd[n].shape) for n in hnames}
    groups = [(g, s, w, [bb[n] for n in ns if n in bb]) for g, s, w, ns in reference_param_groups(net.named_parameters(), WD)] + \
             [(g, s, w, [hd[n] for n in ns]) for g, s, w, ns in head_param_groups(hnames, shapes, WD)]
    topt = torch.optim.AdamW([{"params": ps, "weight_decay": w} for _, _, w, ps in groups if ps], lr=LR, betas=(0.9, 0.999), eps=1e-8)
    for step in range(2):
        head.dropout_mask = masks[step].cuda()
        loss = tr.step(img.cuda(), head.loss_and_grads(lab[step].cuda()))
        torch.cuda.synchronize()
        if step == 0:
            g_bb = {n: tr.flat.view(tr.flat.grad, n).cpu().clone() for n in bb}
            g_hd = {n: tr.hflat.view(tr.hflat.grad, n).cpu().clone() for n in hnames}
            sqn = float(tr.opt.sqn.item())
        feats = O.backbone_forward(img, {**fixed, **bb}, CFG["depth"], CFG["heads"], CFG["interval"], [0, 1, 2, 3])
        ref_loss = torch_seg_loss(torch_uper(hd, feats, head.pool_scales, True, masks[step]), lab[step])
        topt.zero_grad()
        ref_loss.backward()
        assert abs(loss.item() - ref_loss.item()) < 1e-3 * ref_loss.item()
        if step == 0:
            # relative to the larger of the tensor's own scale and 1% of the largest gradient: some gradients are ~0 by construction (the
            # backbone's FPN output biases: every path into the head starts with a training-mode BN, whose backward removes the mean) and hold
            # rounding noise only
            gmax = max(float(bb[n].grad.abs().max()) for n in bb if bb[n].grad is not None)
            for n in bb:
                if bb[n].grad is not None:
                    scale = max(float(bb[n].grad.abs().max()), 1e-2 * gmax)
                    assert float((g_bb[n] - bb[n].grad).abs().max()) < 2e-3 * scale, n
            for n in hnames:
                assert rel_err(g_hd[n], hd[n].grad) < 1e-3, n
            allp = [p for p in list(bb.values()) + [hd[n] for n in hnames] if p.grad is not None]
            total = torch.nn.utils.clip_grad_norm_(allp, MAX_NORM)
            assert total.item() > MAX_NORM        # (clipping active: the joint norm decides the step)
            assert abs(sqn ** 0.5 - total.item()) < 1e-3 * total.item()
        else:
            torch.nn.utils.clip_grad_norm_([p for p in list(bb.values()) + [hd[n] for n in hnames] if p.grad is not None], MAX_NORM)
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
        if n in bb and float(g.abs().max()) < 1e-2 * gmax:      # a gradient of rounding noise (above): Adam moves it by at most lr per step either way
            assert float((ours - ref).abs().max()) <= 2 * 2 * LR + 1e-5, n
            continue
        bad = (ours - ref).abs() > 1e-5 + 1e-3 * LR
        tiny = g.abs() < 5e-3 * g.abs().max()
        assert bool((bad & ~tiny).sum() == 0), "%s: %d elements differ" % (n, int((bad & ~tiny).sum()))
    for k, v in head.state_dict().items():
        if "running" in k:
            assert rel_err(v.cpu(), hd[k]) < 1e-4, k
        elif "num_batches_tracked" in k:
            assert int(v) == 2, k


def test_checkpoint_round_trip_with_head():
    from mtp_amd.parallel import DataParallelTrainer
    params, head, img, lab, masks = _setup(3)
    tr = DataParallelTrainer(_net(params), lr=LR, max_norm=MAX_NORM, feature_dtype=torch.float32, decode_head=head.cuda().train())
    head.dropout_mask = masks[0].cuda()
    tr.step(img.cuda(), head.loss_and_grads(lab[0].cuda()))
    ck = tr.checkpoint()
    assert "decode_head" in ck and set(ck["decode_head"]["state_dict"]) == set(head.state_dict())
    _, head2, _, _, _ = _setup(9)          # another initial state, overwritten by the load
    tr2 = DataParallelTrainer(_net(params), lr=LR, max_norm=MAX_NORM, feature_dtype=torch.float32, decode_head=head2.cuda().train())
    tr2.load_checkpoint(ck)
    for k, v in head.state_dict().items():
        assert torch.equal(v, head2.state_dict()[k]), k
    assert torch.equal(tr.hopt.m, tr2.hopt.m) and torch.equal(tr.hopt.v, tr2.hopt.v) and tr2.hopt.t == tr.hopt.t == 1
    assert torch.equal(tr.hflat.data, tr2.hflat.data)
    for t in (tr, tr2):
        t.module.train()
    head.dropout_mask, head2.dropout_mask = masks[1].cuda(), masks[1].cuda()
    tr.step(img.cuda(), head.loss_and_grads(lab[1].cuda()))
    tr2.step(img.cuda(), head2.loss_and_grads(lab[1].cuda()))
    torch.cuda.synchronize()
    assert rel_err(tr2.hflat.data.cpu(), tr.hflat.data.cpu()) < 1e-5 and rel_err(tr2.flat.data.cpu(), tr.flat.data.cpu()) < 1e-5


def _plain_loss(feats):
    loss = sum(f.float().mean() for f in feats)
    return loss, [torch.full_like(f, 1.0 / f.numel()) for f in feats]


def test_step_without_head_is_unchanged():
    """decode_head=None: the same step, bit for bit, as a trainer built without the keyword, and no head state anywhere"""
    from mtp_amd.parallel import DataParallelTrainer
    params, _, img, _, _ = _setup()
    out = []
    for kw in ({}, {"decode_head": None}):
        torch.manual_seed(0)
        tr = DataParallelTrainer(_net(params), lr=LR, max_norm=1.0, feature_dtype=torch.float32, **kw)
        for _ in range(2):
            tr.step(img.cuda(), _plain_loss)
        torch.cuda.synchronize()
        assert tr.head is None and tr.hflat is None and "decode_head" not in tr.checkpoint()
        out.append((tr.flat.data.clone(), tr.opt.m.clone(), tr.opt.v.clone()))
    for a, b in zip(*out):       # (two runs of one configuration differ in the last bits: f32-atomic sums in a few gradient by-products)
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
