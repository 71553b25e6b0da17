"""GPU: layer-wise lr decay in the fused AdamW -- mtp_adamw_flat_lr / mtp_adamw_weight_images_lr against torch.optim.AdamW with a per-group
lr (+ clip_grad_norm_), FlatAdamW with layer-decay groups on a ViT and an InternImage, and one DataParallelTrainer step with the
reference's pretraining presets."""
import ctypes as C
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 5.0
# (shape, images, f32_out): matrices with images in the activation dtype or (f32_out) in f32, and 1-D parameters as rows of 64 without images.  The image
# writer takes its element-wise path when a dimension is no multiple of the 16-byte store (8 bf16 / 4 f32), so (12, 20) is element-wise for bf16 images and on
# the vector path, with 4-wide ragged edges both ways, for f32 ones -- as the activation dtype (KINDS) and as f32_out; (10, 6) and (6, 10) are element-wise always.
SHAPES = [((64, 128), True, False), ((300,), False, False), ((72, 200), True, True), ((8, 16), True, False), ((1000,), False, False), ((12, 20), True, False),
          ((136, 64), True, False), ((4,), False, False), ((96, 64), False, False), ((2048,), False, False), ((40, 8), True, False), ((128, 72), True, False),
          ((64,), False, False), ((24, 24), True, False), ((777,), False, False), ((16, 256), True, False), ((32, 32), False, False), ((130,), False, False),
          ((8, 8), True, False), ((256, 16), True, False), ((12, 20), True, True), ((10, 6), True, False), ((6, 10), True, True)]
# kind -> (entry point family, activation dtype of the images)
KINDS = {"flat": ("flat", torch.bfloat16), "images": ("images", torch.bfloat16), "images_f32": ("images", torch.float32)}


def _layout():
    off, segs = 0, []
    for shape, img, f32_out in SHAPES:
        numel = 1
        for s in shape:
            numel *= s
        segs.append((off, shape, numel, img, f32_out))
        off += (numel + 63) // 64 * 64
    return segs, off


def _scales(k, ones=False):
    g = torch.Generator().manual_seed(11)
    sc = [1.0] * k if ones else [0.9 ** int(e) for e in torch.randint(0, 26, (k,), generator=g)]
    wd = [0.0 if len(s) == 1 else 0.05 * (1 + i % 3) for i, (s, _, _) in enumerate(SHAPES)]
    return sc, wd


def _descs(segs, p, images, wd):
    from mtp_amd import _lib
    arr = (_lib.WimgDesc * len(segs))()
    tile0 = 0
    for i, (off, shape, numel, img, f32_out) in enumerate(segs):
        R, Cc = shape if len(shape) == 2 else ((numel + 63) // 64, 64)
        d = arr[i]
        d.src = p.data_ptr() + 4 * off
        d.w, d.wt = (images[i][0].data_ptr(), images[i][1].data_ptr()) if img else (None, None)
        d.R, d.C, d.tile0, d.f32_out, d.wd = R, Cc, tile0, int(f32_out), wd[i]
        tile0 += ((R + 63) // 64) * ((Cc + 63) // 64)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), tile0


@functools.lru_cache(maxsize=None)
def _run(kind, ones=False, plain=False, steps=3):
    """kind (KINDS): three steps of the HIP entry point over random flat buffers (23 segments); returns (p, m, v, images, views, torch reference params, scales).
    Cached: every test reads the results, none changes them."""
    from mtp_amd import _lib
    lib = _lib.load()
    family, act = KINDS[kind]
    segs, total = _layout()
    sc, wd = _scales(len(segs), ones)
    g0 = torch.Generator().manual_seed(5)
    p = torch.zeros(total, device="cuda")
    views = []
    for off, shape, numel, _, _ in segs:
        p[off:off + numel] = torch.randn(numel, generator=g0).cuda()
        views.append((off, shape, numel))
    m, v, grad = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    ref = [p[o:o + n].view(s).clone() for o, s, n in views]
    topt = torch.optim.AdamW([{"params": [q], "lr": LR * s, "weight_decay": w} for q, s, w in zip(ref, sc, wd)], lr=LR, betas=BETAS, eps=EPS)
    images = [tuple(torch.zeros(sh, device="cuda", dtype=torch.float32 if f32_out else act) for sh in (shape, shape[::-1])) if img else None
              for _, shape, _, img, f32_out in segs]
    table, tiles = _descs(segs, p, images, wd)
    seg_start = torch.tensor([sg[0] for sg in segs], dtype=torch.int64, device="cuda")
    seg_wd = torch.tensor(wd, dtype=torch.float32, device="cuda")
    seg_lr = torch.tensor(sc, dtype=torch.float32, device="cuda")
    sqn = torch.zeros(1, device="cuda")
    hyper = torch.zeros(6, device="cuda")
    for t in range(1, steps + 1):
        grad.zero_()
        for (o, s, n), q in zip(views, ref):
            gv = torch.randn(n, generator=g0)
            grad[o:o + n] = gv.cuda()
            q.grad = gv.view(s).cuda()
        sqn.fill_(float((grad.double() ** 2).sum()))        # (deterministic: the f32-atomic ops.sqnorm differs in the last bits from run to run)
        hyper.copy_(torch.tensor([LR, BETAS[0], BETAS[1], EPS, 1 - BETAS[0] ** t, 1 - BETAS[1] ** t]))
        st = torch.cuda.current_stream().cuda_stream
        if family == "flat":
            lrs = [] if plain else [seg_lr.data_ptr()]
            fn = lib.mtp_adamw_flat if plain else lib.mtp_adamw_flat_lr
            rc = fn(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), total, seg_start.data_ptr(), seg_wd.data_ptr(), *lrs, len(segs),
                    hyper.data_ptr(), sqn.data_ptr(), C.c_float(MAX_NORM), C.c_float(1.0), st)
        else:
            lrs = [] if plain else [seg_lr.data_ptr()]
            fn = lib.mtp_adamw_weight_images if plain else lib.mtp_adamw_weight_images_lr
            rc = fn(table.data_ptr(), *lrs, len(segs), tiles, _lib.MTP_F32 if act == torch.float32 else _lib.MTP_BF16, p.data_ptr(), grad.data_ptr(), m.data_ptr(),
                    v.data_ptr(), hyper.data_ptr(), sqn.data_ptr(), C.c_float(MAX_NORM), C.c_float(1.0), st)
        assert rc == 0
        norm = torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
        assert float(norm) > 2 * MAX_NORM            # clipping is active
        topt.step()
    torch.cuda.synchronize()
    return p, m, v, images, views, ref, sc


def _assert_images_are_the_cast_master(p, images, views):
    """both images of every matrix equal the updated master cast to the image's dtype (bf16 / f32 activations, or f32 where the descriptor says f32_out)"""
    seen = set()
    for (o, s, n), im in zip(views, images):
        if im is not None:
            pv = p[o:o + n].view(s)
            assert torch.equal(im[0], pv.to(im[0].dtype)) and torch.equal(im[1], pv.t().contiguous().to(im[1].dtype)), (s, im[0].dtype)
            seen.add(im[0].dtype)
    return seen


@pytest.mark.parametrize("kind", list(KINDS))
def test_lr_entry_points_match_torch_adamw_with_per_group_lr(kind):
    p, m, v, images, views, ref, sc = _run(kind)
    assert len(set(sc)) > 5
    worst = 0.0
    for (o, s, n), q in zip(views, ref):
        worst = max(worst, rel_err(p[o:o + n].view(s), q.detach()))
    assert worst <= 2e-6, worst
    if KINDS[kind][0] == "images":
        assert _assert_images_are_the_cast_master(p, images, views) == {KINDS[kind][1], torch.float32}
    # the 64-element padding of every parameter stays zero
    used = torch.zeros_like(p, dtype=torch.bool)
    for o, s, n in views:
        used[o:o + n] = True
    assert float(p[~used].abs().max()) == 0.0


@pytest.mark.parametrize("kind", list(KINDS))
def test_lr_entry_points_with_unit_scales_equal_the_plain_ones_bit_for_bit(kind):
    a = _run(kind, ones=True)
    b = _run(kind, ones=True, plain=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    if KINDS[kind][0] == "images":
        for x, y in zip(a[3], b[3]):
            assert x is None or (torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]))


@pytest.mark.parametrize("plain", [False, True], ids=["lr", "plain"])
@pytest.mark.parametrize("kind", ["images", "images_f32"])
def test_fused_entry_points_leave_the_state_of_the_flat_ones_bit_for_bit(kind, plain):
    """mtp_adamw_weight_images[_lr] against mtp_adamw_flat[_lr] from the same state: parameters and both moments bit for bit after three steps (one AdamW update
    in the library, whatever path writes the images), and the images of the plain form are the cast master too"""
    a = _run(kind, ones=plain, plain=plain)
    b = _run("flat", ones=plain, plain=plain)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert _assert_images_are_the_cast_master(a[0], a[3], a[4]) == {KINDS[kind][1], torch.float32}


def _vit(depth=4):
    import mtp_amd
    torch.manual_seed(5)
    net = mtp_amd.ViT_Win_RVSA_V3_WSZ7(img_size=224, embed_dim=128, depth=depth, num_heads=2, interval=2, qkv_bias=True, use_abs_pos_emb=True,
                                       out_indices=list(range(depth)), drop_path_rate=0.0, precision="bf16")
    with torch.no_grad():
        for n, q in net.named_parameters():
            if "rel_pos" in n:
                q.normal_(0, 0.02)
    return net.cuda().train()


def _internimage():
    import mtp_amd
    import recipe
    c = recipe.II_CFG
    torch.manual_seed(3)
    net = mtp_amd.InternImage(channels=c["channels"], depths=c["depths"], groups=c["groups"], layer_scale=c["layer_scale"], offset_scale=c["offset_scale"],
                              post_norm=True, drop_path_rate=0.0, precision="bf16")
    with torch.no_grad():
        for n, q in net.named_parameters():
            if ".dcn.offset.weight" in n or ".dcn.mask.weight" in n:
                q.normal_(0, 0.02)
    return net.cuda().train()


@pytest.mark.parametrize("model,fused", [("vit", "1"), ("vit", "0"), ("internimage", "1")])
def test_flat_adamw_with_layer_decay_groups_matches_torch_adamw(model, fused, monkeypatch):
    from mtp_amd.optim_groups import pretrain_optim_wrapper
    from mtp_amd.parallel import DataParallelTrainer
    monkeypatch.setenv("MTP_FUSED_ADAMW", fused)
    if model == "vit":
        net, prefix, ow = _vit(), "backbone.", pretrain_optim_wrapper("vit_b")
        ow["paramwise_cfg"]["num_layers"] = 4
    else:
        import recipe
        net, prefix, ow = _internimage(), "encoder.", pretrain_optim_wrapper("internimage_xl")
        ow["paramwise_cfg"].update(num_layers=sum(recipe.II_CFG["depths"]), depths=recipe.II_CFG["depths"])
    ow["optimizer"]["lr"] = LR
    tr = DataParallelTrainer(net, max_norm=1.0, optim_wrapper=ow, param_prefix=prefix)
    f, opt = tr.flat, tr.opt
    assert len(set(s for _, s, _, _ in opt.param_groups)) > 3
    tr.engine.prepare_weights()
    opt.fuse_images(tr.engine._wimg)
    if model == "vit":            # (InternImage: whether its images qualify for the fused form is the engine's business)
        assert (opt._fused is not None) == (fused == "1")
    trained = [n for n in f.names if f.groups[n] is not None]
    ref = {n: f.view(f.data, n).detach().clone() for n in trained}
    p0 = {n: q.clone() for n, q in ref.items()}
    of = {n: (s, w) for _, s, w, ns in opt.param_groups for n in ns}
    topt = torch.optim.AdamW([{"params": [ref[n]], "lr": LR * of[n][0], "weight_decay": of[n][1]} for n in trained], lr=LR, betas=BETAS, eps=EPS)
    g0 = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(3):
        f.grad.zero_()
        for n in trained:
            gv = f.view(f.grad, n)
            gv.copy_(torch.randn(gv.shape, generator=g0, device="cuda"))
            ref[n].grad = gv.clone()
        opt.step()
        torch.nn.utils.clip_grad_norm_(list(ref.values()), 1.0)
        topt.step()
    torch.cuda.synchronize()
    # compared as updates, to 2e-5 of the largest update + 4 f32 ulps of the parameter (three roundings of p + update on each side): the kernels take beta2 as
    # f32, and 1 - f32(0.999) is 1.3e-5 below 1e-3, so every step is 6.4e-6 longer than torch's (which forms 1 - beta2 in double) -- invisible against a
    # parameter of size 1, but the whole value of a zero-initialised bias after three steps
    errs = []
    for n in trained:
        d, dr = f.view(f.data, n) - p0[n], ref[n] - p0[n]
        tol = 2e-5 * float(dr.abs().max()) + 4 * torch.finfo(torch.float32).eps * float(ref[n].abs().max())
        errs.append((float((d - dr).abs().max()) / tol, n))
    errs.sort(reverse=True)
    assert errs[0][0] <= 1.0, errs[:4]


@pytest.mark.parametrize("model", ["vit", "internimage"])
def test_trainer_step_with_the_pretraining_preset_scales_block_updates(model):
    from mtp_amd.optim_groups import pretrain_optim_wrapper
    from mtp_amd.parallel import DataParallelTrainer
    if model == "vit":
        net, prefix, ow = _vit(), "backbone.", pretrain_optim_wrapper("vit_b")
        first, last = "blocks.0.mlp.fc1.weight", "blocks.3.mlp.fc1.weight"
        img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3)).cuda()
    else:
        net, prefix, ow = _internimage(), "encoder.", pretrain_optim_wrapper("internimage_xl")
        first, last = "levels.0.blocks.0.mlp.fc1.weight", "levels.3.blocks.0.mlp.fc1.weight"
        img = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(4)).cuda()
    tr = DataParallelTrainer(net, optim_wrapper=ow, param_prefix=prefix)
    P = dict(net.named_parameters())
    before = {n: P[n].detach().clone() for n in (first, last)}

    def lg(feats):
        gs = [torch.randn(f.shape, generator=torch.Generator().manual_seed(20 + i)).to(f.device, f.dtype) for i, f in enumerate(feats)]
        return sum((f.float() * g.float()).sum() for f, g in zip(feats, gs)), gs
    tr.step(img, lg)
    torch.cuda.synchronize()
    scale = {n: s for _, s, _, ns in tr.opt.param_groups for n in ns}
    want = scale[first] / scale[last]
    assert want < 0.75
    d0 = (P[first].detach() - before[first]).abs().median().item()
    d1 = (P[last].detach() - before[last]).abs().median().item()
    assert d1 > 0 and abs(d0 / d1 - want) <= 0.05 * want, (d0, d1, want)
