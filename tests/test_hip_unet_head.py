"""GPU: change detection on the kernels of csrc/unet_head.hip and the engine of mtp_amd/engine_unet.py, under the guard arena.
  * the kernels (pair fusion, the UNet decoder block's upsample + concatenate) bit for bit against torch and against the resize kernels they share
    their index rule with; mtp_seg_ce with logits FINER than the labels (the ViT configs: 512^2 logits for 256^2 labels), which no other test covers;
  * the whole head (fp32 mode) against the torch restatement of tests/unet_ref.py in float64 and against the reference's own head (fixture f19),
    through autograd and through loss_and_grads, with and without the pair fusion; bf16 mode against torch's own bf16-autocast error; eval-mode
    predict; SyncBN's exchange hook with two emulated ranks."""
import pytest
import torch
import torch.nn.functional as F

import guard
from conftest import rel_err
from mtp_amd import ops

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
ARENA = None


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    global ARENA
    ARENA = a = guard.Arena("cuda")
    monkeypatch.setattr(ops, "_scratch", a.scratch)
    yield a
    ARENA = None
    torch.cuda.synchronize()
    try:
        a.check()
    finally:
        a.close()


def to_rows(x):
    """NCHW -> (N*H*W, C)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def dyadic(shape, g):
    """multiples of 1/8 in [-8, 8]: sums of a few of them are exact in f32 and they are bf16 numbers"""
    return torch.randint(-64, 65, shape, generator=g).float() / 8


def in_slice(t, pad=4, dtype=None):
    """a frozen device copy of the 2-D map t living as a column slice of a wider buffer (pitch > width)"""
    w = ARENA.wide(t.shape[0], t.shape[1] + 2 * pad, dtype=dtype or t.dtype)
    s = ARENA.cols(w, pad, pad + t.shape[1])
    s.copy_(t)
    ARENA.frozen(w)
    return s


def out_slice(rows, cols, dtype, pad=4):
    w = ARENA.wide(rows, cols + 2 * pad, dtype=dtype)
    return ARENA.cols(w, pad, pad + cols)


def torch_fuse(x1, x2, policy):
    return {"concat": lambda: torch.cat([x1, x2], 1), "sum": lambda: x1 + x2, "diff": lambda: x2 - x1, "abs_diff": lambda: (x1 - x2).abs()}[policy]()


FUSE_SHAPES = [(2, 8, 1, 2), (4, 24, 3, 5), (2, 1024, 16, 16)]


def _pair_input(shape, dt, g):
    B, C, H, W = shape
    f = torch.randn(B, C, H, W, generator=g).to(dt)
    same = torch.rand(B // 2, C, H, W, generator=g) < 0.25          # pixels where x1 == x2 exactly
    f[B // 2:][same] = f[:B // 2][same]
    return f


@pytest.mark.parametrize("policy", ["abs_diff", "diff", "sum", "concat"])
@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F32, BF16)])
@pytest.mark.parametrize("shape", FUSE_SHAPES)
def test_fuse_pair_forward_is_bit_equal_to_torch(shape, in_dt, out_dt, policy):
    B, C, H, W = shape
    N = B // 2
    f = _pair_input(shape, in_dt, torch.Generator().manual_seed(C + H))
    ref = to_rows(torch_fuse(f[:N], f[N:], policy)).to(out_dt)
    fd = ARENA.frozen(ARENA.like(f))
    out = ops.fuse_pair_fwd(fd, out_slice(N * H * W, ref.shape[1], out_dt), policy)
    assert torch.equal(out.cpu(), ref)
    ARENA.check()        # the columns on both sides of the slice are still poison


@pytest.mark.parametrize("policy", ["abs_diff", "diff", "sum", "concat"])
@pytest.mark.parametrize("in_dt", [F32, BF16])
@pytest.mark.parametrize("shape", FUSE_SHAPES)
def test_fuse_pair_backward_is_bit_equal_to_autograd(shape, in_dt, policy):
    B, C, H, W = shape
    N = B // 2
    g = torch.Generator().manual_seed(C + W)
    f = _pair_input(shape, in_dt, g)
    x = f.clone().requires_grad_(True)
    y = torch_fuse(x[:N], x[N:], policy)
    gr = dyadic(y.shape, g)
    y.backward(gr.to(in_dt))
    fd = ARENA.frozen(ARENA.like(f))
    df = ops.fuse_pair_bwd(in_slice(to_rows(gr)), fd, ARENA.empty(B, C, H, W), policy)
    assert torch.equal(df.cpu(), x.grad.float())
    if policy == "abs_diff":
        same = (f[:N] == f[N:])
        assert same.any() and df.cpu()[:N][same].abs().max() == 0 and df.cpu()[N:][same].abs().max() == 0


# (h, w) of x, (hs, ws) of the skip: 1x2 -> 2x4 against 2x3 (a real resize, the fixture's pyramid), x2 (plain enlargement), same size (copies), x16
UP_CASES = [(1, 2, 2, 3), (3, 5, 3, 5), (8, 8, 16, 16), (16, 16, 2, 2)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("h,w,hs,ws", UP_CASES)
def test_up_cat_forward_is_bit_equal_to_nearest_and_to_the_resize_kernel(h, w, hs, ws, dt):
    N, Cx, Cs = 2, 8, 12
    g = torch.Generator().manual_seed(h * 7 + ws)
    x, sk = torch.randn(N, Cx, h, w, generator=g).to(dt), torch.randn(N, Cs, hs, ws, generator=g).to(dt)
    xd, sd = in_slice(to_rows(x)), in_slice(to_rows(sk))
    rows = N * 4 * h * w
    y = ops.unet_up_cat_fwd(xd, sd, out_slice(rows, Cx + Cs, dt), N, h, w, hs, ws)
    assert torch.equal(y[:, :Cx].cpu(), to_rows(F.interpolate(x.float(), scale_factor=2, mode="nearest")).to(dt))
    ref = ops.resize_bilinear_fwd(sd, out_slice(rows, Cx + Cs, dt)[:, Cx:], N, hs, ws, 2 * h, 2 * w)
    assert torch.equal(y[:, Cx:], ref)
    assert rel_err(y[:, Cx:].float().cpu(), to_rows(F.interpolate(sk.float(), size=(2 * h, 2 * w), mode="bilinear", align_corners=False))) < (1e-5 if dt == F32 else 8e-3)
    if (hs, ws) == (2 * h, 2 * w):
        assert torch.equal(y[:, Cx:].cpu(), to_rows(sk))
    # the skip-less last block (Cs = 0), into a wider map
    y0 = ops.unet_up_cat_fwd(xd, None, out_slice(rows, Cx, dt), N, h, w)
    assert torch.equal(y0, y[:, :Cx])
    # f32 operands into a bf16 map (the engine's fp32 -> bf16 seam does not exist today; the dispatch does)
    if dt == F32:
        yb = ops.unet_up_cat_fwd(xd, sd, out_slice(rows, Cx + Cs, BF16), N, h, w, hs, ws)
        assert torch.equal(yb, y.to(BF16))
    ARENA.check()


@pytest.mark.parametrize("h,w,hs,ws", UP_CASES)
def test_up_cat_backward_is_bit_equal_to_autograd_and_to_the_resize_kernel(h, w, hs, ws):
    N, Cx, Cs = 2, 8, 12
    g = torch.Generator().manual_seed(h * 11 + ws)
    rows = N * 4 * h * w
    dy = dyadic((N, Cx + Cs, 2 * h, 2 * w), g)
    dyd = in_slice(to_rows(dy))
    x = torch.zeros(N, Cx, h, w, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(dy[:, :Cx])
    dx, dsk = ops.unet_up_cat_bwd(dyd, out_slice(N * h * w, Cx, F32), out_slice(N * hs * ws, Cs, F32), N, h, w, hs, ws)
    assert torch.equal(dx.cpu(), to_rows(x.grad))
    ref = ops.resize_bilinear_bwd(dyd[:, Cx:], ARENA.empty(N * hs * ws, Cs), N, hs, ws, 2 * h, 2 * w)
    assert torch.equal(dsk, ref)
    # accumulate adds onto preset values (dyadic: the sums stay exact)
    px, ps = dyadic((N * h * w, Cx), g), torch.randn(N * hs * ws, Cs, generator=g)
    ax, asx = out_slice(N * h * w, Cx, F32), out_slice(N * hs * ws, Cs, F32)
    ax.copy_(px)
    asx.copy_(ps)
    ops.unet_up_cat_bwd(dyd, ax, asx, N, h, w, hs, ws, accumulate=True)
    assert torch.equal(ax.cpu(), px + to_rows(x.grad))
    ref2 = ARENA.like(ps)
    ops.resize_bilinear_bwd(dyd[:, Cx:], ref2, N, hs, ws, 2 * h, 2 * w, accumulate=True)
    assert torch.equal(asx, ref2)
    # the skip-less block, and two runs on arbitrary values bit-identical
    d0 = ops.unet_up_cat_bwd(dyd[:, :Cx], ARENA.empty(N * h * w, Cx), None, N, h, w)[0]
    assert torch.equal(d0, dx)
    dr = in_slice(torch.randn(rows, Cx + Cs, generator=g))
    a = ops.unet_up_cat_bwd(dr, ARENA.empty(N * h * w, Cx), ARENA.empty(N * hs * ws, Cs), N, h, w, hs, ws)
    b = ops.unet_up_cat_bwd(dr, ARENA.empty(N * h * w, Cx), ARENA.empty(N * hs * ws, Cs), N, h, w, hs, ws)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert rel_err(a[0].cpu(), dr[:, :Cx].cpu().reshape(N, h, 2, w, 2, Cx).sum((2, 4)).reshape(-1, Cx)) < 1e-6
    ARENA.check()


def test_fuse_and_up_cat_reject_bad_arguments():
    f = torch.zeros(2, 8, 2, 2, device="cuda")
    with pytest.raises(ValueError):
        ops.fuse_pair_fwd(f, torch.zeros(4, 8, device="cuda"), "max")
    with pytest.raises(ops._lib.MtpHipError):       # 6 channels: not a multiple of 4
        ops.fuse_pair_fwd(torch.zeros(2, 6, 2, 2, device="cuda"), torch.zeros(4, 6, device="cuda"), "sum")
    with pytest.raises(ops._lib.MtpHipError):       # 6 columns
        ops.unet_up_cat_fwd(torch.zeros(4, 6, device="cuda"), None, torch.zeros(16, 6, device="cuda"), 1, 2, 2)


@pytest.mark.parametrize("N,H,K", [(2, 5, 2), (2, 16, 2)])
def test_seg_loss_with_logits_finer_than_the_labels(N, H, K):
    """h = 2H: the loss's resize SHRINKS the logits (x2 up in the head followed by x2 down here is a 3-tap blur, not the identity); loss and gradient
    against torch at test_seg_loss_against_torch's tolerances"""
    g = torch.Generator().manual_seed(N + H + K)
    h = 2 * H
    logits = torch.randn(N, K, h, h, generator=g, dtype=torch.float64, requires_grad=True)
    lab = torch.randint(0, K, (N, H, H), generator=g)
    lab[torch.rand(N, H, H, generator=g) < 0.2] = 255
    up = F.interpolate(logits, size=(H, H), mode="bilinear", align_corners=False)
    ref = 0.7 * F.cross_entropy(up, lab, ignore_index=255, reduction="sum") / lab.numel()
    ref.backward()
    Kp = ops.pad8(K)
    lr = torch.zeros(N * h * h, Kp, device="cuda")
    lr[:, :K] = to_rows(logits.detach()).float()
    labd = lab.to("cuda", torch.uint8)
    ARENA.frozen(lr, labd)
    loss, dl = ops.seg_ce(lr, K, N, h, h, labd, 255, 0.7)
    print("seg_ce h=2H: loss %.8g ref %.8g, dlogits rel err %.3g" % (loss.item(), ref.item(), rel_err(dl[:, :K].cpu(), to_rows(logits.grad))))
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert rel_err(dl[:, :K].cpu(), to_rows(logits.grad)) < 1e-4
    assert dl[:, K:].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------ the whole head
import unet_ref as R                      # noqa: E402
from mtp_amd import UNetHead              # noqa: E402
from mtp_amd.engine_decode import DecodeEngine      # noqa: E402

# (geometry, im2col chunk budget in bytes): the default (every 3x3 layer in one chunk), and at B = 2 a budget below one sample's columns, so every
# 3x3 layer works one sample per chunk: 2 chunks, the weight gradient's first chunk written in place and the second added through `tmp`
CHUNKED = dict(argnames="tag,budget", argvalues=[("flat", None), ("pyr", None), ("pyr", 1)], ids=["flat", "pyr", "pyr-chunked"])


def _budget(monkeypatch, budget):
    """lower the budget and watch the head's own 3x3 layers: -> the (samples, chunks) of every forward / backward call of one"""
    seen = []
    if budget is not None:
        orig = DecodeEngine._chunks

        def watched(self, N, HW, Kp):
            chunks = orig(self, N, HW, Kp)
            seen.append((N, len(chunks)))
            return chunks
        monkeypatch.setattr(DecodeEngine, "COLS_BUDGET", budget)
        monkeypatch.setattr(DecodeEngine, "_chunks", watched)
    return seen


def _randomise_bn(head, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, t in head.state_dict(keep_vars=True).items():
            if n.endswith(".1.weight"):
                t.copy_(1.0 + 0.2 * torch.randn(t.shape, generator=g))
            elif n.endswith(".1.bias") or n.endswith("running_mean") or n == "conv_seg.bias":
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
            elif n.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif n == "conv_seg.weight":
                t.copy_(0.05 * torch.randn(t.shape, generator=g))
    return head


def _case(tag, seed=0, B=2, pairs=None, **kw):
    """a seeded head and batch at fixture f19's geometry `tag` whose ReLU pre-activations all keep 2e-5 away from 0 (closer, an f32 forward may take
    the other side of the kink than the float64 reference: a property of the data, not of the code).  pairs: a fusion policy -- the inputs are then
    the 2B-batch maps and the margin is taken on the fused maps."""
    chans, sizes, lab_size = R.F19_GEOMS[tag]
    cin = [c // 2 for c in chans] if pairs == "concat" else chans
    for attempt in range(50):
        torch.manual_seed(seed)
        head = _randomise_bn(UNetHead(**dict(R.F19_HEAD, in_channels=chans, encoder_channels=chans, **kw)), seed + 1)
        g = torch.Generator().manual_seed(seed + 7 + 1000 * attempt)
        ins = [torch.randn(B * (2 if pairs else 1), c, *s, generator=g) for c, s in zip(cin, sizes)]
        lab = torch.randint(0, 2, (B,) + lab_size, generator=g)
        lab[torch.rand(lab.shape, generator=g) < 0.15] = 255
        mask = (torch.rand(B, head.channels, generator=g) >= 0.1).float() / 0.9
        mask[0, 1] = 0.0
        fused = [R.torch_fuse(x[:B], x[B:], pairs) for x in ins] if pairs else ins
        R.probe = []
        sd = {k: v.double() if v.is_floating_point() else v.clone() for k, v in head.state_dict().items()}
        with torch.no_grad():
            R.torch_unet_feature(sd, [x.double() for x in fused], 4, True)
        margin, R.probe = min(R.probe), None
        if margin > 2e-5:
            return head, ins, lab, mask
    raise AssertionError("no seed with a ReLU margin")


def _reference(head, ins, lab, mask, dtype=torch.float64, pairs=None):
    sd = {k: v.detach().clone().to(dtype if v.is_floating_point() else v.dtype).requires_grad_(v.is_floating_point() and "running" not in k)
          for k, v in head.state_dict().items()}
    xi = [x.to(dtype).requires_grad_(True) for x in ins]
    B = lab.shape[0]
    fused = R.torch_neck([x[:B] for x in xi], [x[B:] for x in xi], pairs) if pairs else xi
    logits = R.torch_unet(sd, fused, 4, True, mask.to(dtype))
    loss = R.torch_seg_loss(logits, lab)
    loss.backward()
    return logits.detach(), loss.detach(), [x.grad for x in xi], sd


def _assert_grads(h, sd, tol=1e-3):
    for n, p in h.named_parameters():
        assert rel_err(p.grad.cpu(), sd[n].grad) < tol, n


@pytest.mark.parametrize(**CHUNKED)
def test_head_fp32_against_torch_restatement(tag, budget, monkeypatch):
    seen = _budget(monkeypatch, budget)
    head, ins, lab, mask = _case(tag)
    logits_ref, loss_ref, dins_ref, sd = _reference(head, ins, lab, mask)
    h = head.cuda().train()
    h.dropout_mask = mask.cuda()
    xi = [x.cuda().requires_grad_(True) for x in ins]
    logits = h(xi)
    loss = h.loss_by_feat(logits, lab.cuda().to(torch.uint8))["loss_ce"]
    loss.backward()
    assert logits.shape == logits_ref.shape and rel_err(logits.detach().cpu(), logits_ref) < 1e-3
    assert abs(loss.item() - loss_ref.item()) < 1e-3 * loss_ref.item()
    for a, b in zip(xi, dins_ref):
        assert rel_err(a.grad.cpu(), b) < 1e-3
    _assert_grads(h, sd)
    for n, b in h.named_buffers():
        if "running" in n:
            assert rel_err(b.cpu(), sd[n]) < 1e-5, n
        elif "num_batches_tracked" in n:
            assert b.item() == 1, n
    # eval mode (the running statistics, no dropout); predict = those logits resized to a given size; logit_rows = the same as rows
    h.eval()
    with torch.no_grad():
        ev = h([x.cuda() for x in ins]).cpu()
        sde = {k: v.detach().double().cpu() if v.is_floating_point() else v.cpu() for k, v in h.state_dict().items()}
        ev_ref = R.torch_unet(sde, [x.double() for x in ins], 4, False)
    assert rel_err(ev, ev_ref) < 1e-3
    pr = h.predict([x.cuda() for x in ins], (37, 41)).cpu()
    assert rel_err(pr, F.interpolate(ev_ref, size=(37, 41), mode="bilinear", align_corners=False)) < 1e-3
    rows_, (N, H, W) = h.logit_rows([x.cuda() for x in ins])
    assert (N, H, W) == (ev.shape[0], ev.shape[2], ev.shape[3]) and rows_.shape == (N * H * W, 8) and rows_[:, 2:].abs().max().item() == 0
    assert torch.equal(rows_[:, :2].cpu(), to_rows(ev))
    # the trunk alone
    h.train()
    feat = h._forward_feature([x.cuda() for x in ins])
    sdt = {k: v.detach().double().cpu() if v.is_floating_point() else v.cpu() for k, v in h.state_dict().items()}
    assert rel_err(feat.detach().cpu(), R.torch_unet_feature(sdt, [x.double() for x in ins], 4, True)) < 1e-3
    assert budget is None or (len(seen) >= 16 and set(seen) == {(2, 2)}), seen      # every 3x3 layer, forward and backward: 2 chunks of one sample


@pytest.mark.parametrize("tag", ["flat", "pyr"])
def test_head_fp32_against_reference_fixture_f19(golden, tag):
    """fixture f19 = the reference's UNetHead (opencd unet_head.py) in float64: training-mode logits, loss, d(inputs), every parameter gradient, the
    updated running statistics and counters; eval-mode logits -- within 1e-3 relative in fp32 mode"""
    d = golden("f19_unet.npz")
    sd, ins, lab, mask = R.f19_case(golden, tag, torch.float32)
    chans = R.F19_GEOMS[tag][0]
    h = UNetHead(**dict(R.F19_HEAD, in_channels=chans, encoder_channels=chans))
    h.load_state_dict(sd, strict=True)
    h = h.cuda().train()
    h.dropout_mask = mask.cuda()
    xi = [x.cuda().requires_grad_(True) for x in ins]
    logits = h(xi)
    loss = h.loss_by_feat(logits, lab.cuda())["loss_ce"]
    loss.backward()
    assert rel_err(logits.detach().cpu(), torch.from_numpy(d[tag + ".logits_train"])) < 1e-3
    assert abs(loss.item() - float(d[tag + ".loss"])) < 1e-3 * float(d[tag + ".loss"])
    for i, x in enumerate(xi):
        assert rel_err(x.grad.cpu(), torch.from_numpy(d[tag + ".dinput%d" % i])) < 1e-3
    for n, p in h.named_parameters():
        assert rel_err(p.grad.cpu(), torch.from_numpy(d[tag + ".grad." + n])) < 1e-3, n
    for n, b in h.named_buffers():
        ref = torch.from_numpy(d[tag + ".after." + n])
        assert (int(b) == int(ref)) if not ref.is_floating_point() else rel_err(b.cpu(), ref) < 1e-5, n
    h.load_state_dict(sd, strict=True)
    h.eval()
    with torch.no_grad():
        ev = h([x.cuda() for x in ins]).cpu()
    assert rel_err(ev, torch.from_numpy(d[tag + ".logits_eval"])) < 1e-3


@pytest.mark.parametrize(**CHUNKED)
def test_loss_and_grads_fast_path_equals_autograd(tag, budget, monkeypatch):
    seen = _budget(monkeypatch, budget)
    head, ins, lab, mask = _case(tag, seed=3)
    _, loss_ref, dins_ref, sd = _reference(head, ins, lab, mask)
    h = head.cuda().train()
    state = {k: v.clone() for k, v in h.state_dict().items()}
    h.dropout_mask = mask.cuda()
    loss, dins = h.loss_and_grads(lab.cuda())([x.cuda() for x in ins])
    assert abs(loss.item() - loss_ref.item()) < 1e-3 * loss_ref.item()
    for a, b in zip(dins, dins_ref):
        assert rel_err(a.cpu(), b) < 1e-3
    _assert_grads(h, sd)
    # and against the head's own autograd path from the same state: the same kernels in the same order
    fast = {n: p.grad.clone() for n, p in h.named_parameters()}
    h.load_state_dict(state)
    h.zero_grad(set_to_none=True)
    h.dropout_mask = mask.cuda()
    xi = [x.cuda().requires_grad_(True) for x in ins]
    la = h.loss_by_feat(h(xi), lab.cuda())["loss_ce"]
    la.backward()
    assert abs(la.item() - loss.item()) < 1e-6 * loss.item()
    for a, b in zip(xi, dins):
        assert rel_err(a.grad, b) < 1e-5
    for n, p in h.named_parameters():
        assert rel_err(p.grad, fast[n]) < 1e-5, n
    assert budget is None or (len(seen) >= 16 and set(seen) == {(2, 2)}), seen      # every 3x3 layer, forward and backward: 2 chunks of one sample


@pytest.mark.parametrize("tag,policy", [("flat", "abs_diff"), ("pyr", "abs_diff"), ("pyr", "concat"), ("flat", "diff"), ("flat", "sum")])
def test_loss_and_grads_with_fusion_equals_torch_neck_and_head(tag, policy):
    """the training fast path: the backbone's 2N-batch maps in, fused by mtp_fuse_pair_fwd on the way into rows, 2N-batch gradients out -- against the
    torch neck + head under autograd in float64, d(inputs) of both halves included"""
    head, ins, lab, mask = _case(tag, seed=5, pairs=policy)
    _, loss_ref, dins_ref, sd = _reference(head, ins, lab, mask, pairs=policy)
    h = head.cuda().train()
    h.dropout_mask = mask.cuda()
    loss, dins = h.loss_and_grads(lab.cuda(), fusion=policy)([x.cuda() for x in ins])
    assert abs(loss.item() - loss_ref.item()) < 1e-3 * loss_ref.item()
    B = lab.shape[0]
    for a, b in zip(dins, dins_ref):
        assert a.shape == b.shape and a.dtype == F32
        assert rel_err(a.cpu()[:B], b[:B]) < 1e-3 and rel_err(a.cpu()[B:], b[B:]) < 1e-3
    _assert_grads(h, sd)
    with pytest.raises(ValueError):
        h.loss_and_grads(lab.cuda(), fusion="max")


def test_head_bf16_within_torch_autocast_error():
    """bf16 mode against the float64 restatement, bounded by 4x the error of torch's own bf16-autocast run of the restatement on the same inputs
    (measured here; both figures are printed)"""
    head, ins, lab, mask = _case("flat", seed=7)
    logits_ref, loss_ref, dins_ref, sd = _reference(head, ins, lab, mask)
    sdc = {k: v.detach().cuda().float().requires_grad_(v.is_floating_point() and "running" not in k) if v.is_floating_point() else v.cuda()
           for k, v in head.state_dict().items()}
    xa = [x.cuda().requires_grad_(True) for x in ins]
    with torch.autocast("cuda", dtype=BF16):
        la = R.torch_unet(sdc, xa, 4, True, mask.cuda())
    R.torch_seg_loss(la.float(), lab.cuda()).backward()
    e_torch = dict(logits=rel_err(la.detach().float().cpu(), logits_ref), dx=max(rel_err(a.grad.cpu(), b) for a, b in zip(xa, dins_ref)),
                   dw=max(rel_err(sdc[n].grad.cpu(), sd[n].grad) for n, _ in head.named_parameters()))
    h = head.cuda().train()
    h.precision = "bf16"
    h.dropout_mask = mask.cuda()
    xi = [x.cuda().requires_grad_(True) for x in ins]
    logits = h(xi)
    h.loss_by_feat(logits, lab.cuda())["loss_ce"].backward()
    e_ours = dict(logits=rel_err(logits.detach().cpu(), logits_ref), dx=max(rel_err(a.grad.cpu(), b) for a, b in zip(xi, dins_ref)),
                  dw=max(rel_err(p.grad.cpu(), sd[n].grad) for n, p in h.named_parameters()))
    print("bf16 head: ours %s, torch autocast %s" % (e_ours, e_torch))
    for k in e_ours:
        assert e_ours[k] < 4 * e_torch[k], "bf16 %s: ours %.3g, torch autocast %.3g" % (k, e_ours[k], e_torch[k])


def test_syncbn_exchange_with_two_emulated_ranks_equals_whole_batch():
    """the bn_reduce hook: a two-rank all-reduce emulated by running the two half batches in lock step on two threads, through loss_and_grads; each
    rank's d(inputs) equals the whole-batch head's on its half and the ranks' parameter gradients sum to the whole batch's"""
    import threading
    head, ins, lab, mask = _case("pyr", seed=11, B=4, norm_cfg=dict(type="SyncBN", requires_grad=True))
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    whole = head.cuda().train()
    whole.dropout_mask = mask.cuda()
    lw, dw = whole.loss_and_grads(lab.cuda())([x.cuda() for x in ins])
    gw = {n: p.grad.clone() for n, p in whole.named_parameters()}
    chans = R.F19_GEOMS["pyr"][0]
    heads = []
    for _ in range(2):
        h = UNetHead(**dict(R.F19_HEAD, in_channels=chans, encoder_channels=chans, norm_cfg=dict(type="SyncBN")))
        h.load_state_dict(sd)
        heads.append(h.cuda().train())
    bar = threading.Barrier(2)
    slots = [None, None]

    def make(r):
        def red(t):
            slots[r] = t.clone()
            bar.wait()
            s = slots[0] + slots[1]
            bar.wait()
            t.copy_(s)
            return t
        return red
    outs, errs = [None, None], []

    def run(r):
        try:
            torch.cuda.set_device(0)
            heads[r].bn_reduce = make(r)
            heads[r].dropout_mask = mask[2 * r:2 * r + 2].cuda()
            outs[r] = heads[r].loss_and_grads(lab[2 * r:2 * r + 2].cuda())([x[2 * r:2 * r + 2].cuda() for x in ins])
            torch.cuda.synchronize()
        except Exception as ex:      # surfaced below
            errs.append(ex)
            bar.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    # each rank's loss is normalised by its own pixels: (l0 + l1) / 2 = the whole batch's loss; likewise its gradients carry a factor 2
    assert abs((outs[0][0] + outs[1][0]).item() / 2 - lw.item()) < 1e-5 * lw.item()
    for i in range(4):
        assert rel_err((torch.cat([outs[0][1][i], outs[1][1][i]]) / 2).cpu(), dw[i].cpu()) < 1e-4
    for n, g in gw.items():
        tot = (dict(heads[0].named_parameters())[n].grad + dict(heads[1].named_parameters())[n].grad) / 2
        assert rel_err(tot.cpu(), g.cpu()) < 1e-4, n
    for k, v in whole.state_dict().items():
        if "running" in k:
            assert rel_err(heads[0].state_dict()[k].cpu(), v.cpu()) < 1e-5, k
