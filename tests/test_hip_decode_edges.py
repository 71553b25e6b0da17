"""GPU: the kernels of csrc/decode_head.hip and csrc/unet_head.hip where the segmentation heads run them and the op tests did not: on either side of the
BatchNorm partial-chunk seams, in the statistics regimes a one-pass variance fails, at resize ratios near 1 and far from it in both directions, in the
loss's saturated, one-class, 4096-class and many-partials cases and its bf16 instantiations, on the mask rows of Dropout2d, on partial LDS tiles of the
pair fusion, with a skip larger than the decoder block's output, and at the pooling's limit.  Every buffer comes out of the guard arena
(tests/guard.py): outputs NaN-poisoned and between guards, inputs frozen, the wrappers' workspaces (ops._scratch) poisoned and guarded.  Inputs,
references and bounds are tests/decode_cases.py's; tests/test_decode_edges_host.py proves on the CPU what is taken for granted here.

A. BatchNorm chunk seams: integer inputs whose every sum is exact in f32 (proved by the host test), so the statistics kernels return the float64 result
   bit for bit -- a row skipped, counted twice, or a partial row left unwritten (NaN poison) is an unequal number.  bn_apply / bn_bwd_dx at the same
   row counts against float64, the existing tolerances.
B. BatchNorm regimes: bound = max(the project's tolerance, 4 x the error of a float32 restatement of the kernels); both errors are recorded
   (conftest.record_parity, group "decode"; profiles/decode_parity_errors.json holds a run's table).
C. Resize ratios: every ordered pair of decode_cases.Z along one axis, forward, backward (f32 and bf16 dy, accumulating) and the loss's scalar gather.
D. The segmentation loss's regimes and instantiations.  E. channel_scale.  F. Tiles of fuse_pair, up_cat, the pooling."""
import pytest
import torch
import torch.nn.functional as F

import decode_cases as D
import guard
from conftest import record_parity, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
DTN = D.DTN
ARENA = None     # the running test's guard.Arena


@pytest.fixture(scope="module")
def ops():
    from mtp_amd import ops as o
    o.lib()
    return o


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    global ARENA
    from mtp_amd import ops as o
    ARENA = a = guard.Arena("cuda")
    monkeypatch.setattr(o, "_scratch", a.scratch)
    yield a
    ARENA = None
    torch.cuda.synchronize()
    try:
        a.check()
    finally:
        a.close()


def dev(t, dtype=None):
    """an op INPUT: guarded and frozen"""
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t, dtype=None):
    """updated in place by contract: guarded, not frozen"""
    return ARENA.like(t, dtype=dtype or t.dtype)


def e(*shape, dtype=F32):
    """an op OUTPUT: NaN-poisoned, between guards"""
    return ARENA.empty(*shape, dtype=dtype)


def in_slice(t, dtype=None, pad=D.SLICE_PAD):
    """a frozen device copy of the 2-D map t living as a column slice of a wider poisoned buffer (pitch = width + 2 pad)"""
    w = ARENA.wide(t.shape[0], t.shape[1] + 2 * pad, dtype=dtype or t.dtype)
    s = ARENA.cols(w, pad, pad + t.shape[1])
    s.copy_(t)
    ARENA.frozen(w)
    return s


def out_slice(rows, cols, dtype=F32, pad=D.SLICE_PAD):
    w = ARENA.wide(rows, cols + 2 * pad, dtype=dtype)
    return ARENA.cols(w, pad, pad + cols)


def same(got, want, what):
    """got (device) holds the float64 values `want` exactly (bf16: rounded once); NaN, a never-written element, is unequal"""
    g = got.float().cpu()
    w = want.float().to(got.dtype).float()
    bad = ~(g == w)
    assert not bool(bad.any()), "%s: %d of %d elements differ; first at %s: got %r, want %r" % (
        what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(g[bad][0]), float(w[bad][0]))


def still_poison(t):
    view, pat = guard.poison_of(t.dtype)
    return bool((t.view(view) == pat).all())


def watch_scratch(monkeypatch, ops):
    """-> the list of every workspace / self-allocated result the wrappers take from now on"""
    seen = []

    def scratch(shape, device=None, dtype=F32):
        t = ARENA.scratch(shape, device, dtype)
        seen.append(t)
        return t
    monkeypatch.setattr(ops, "_scratch", scratch)
    return seen


# ------------------------------------------------------------------------------------------------ A: chunk seams, bit for bit
@pytest.mark.parametrize("x_dt,dy_dt", [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)], ids=["f32", "bf16", "x_f32-dy_bf16", "x_bf16-dy_f32"])
@pytest.mark.parametrize("C", D.BN_CHANNELS)
@pytest.mark.parametrize("rows", D.BN_ROWS)
def test_bn_statistics_at_chunk_seams_are_exact(ops, rows, C, x_dt, dy_dt):
    """bn_sums (centred and not) and bn_bwd_sums (relu both ways) return the integers: contiguous operands, then column slices of wider frozen buffers.
    The partial-row workspace is poisoned: an empty workgroup that wrote no zeros into its partial row turns the column sums into NaN."""
    c = D.exact_bn_case(rows, C)
    center, mean, rstd, gamma, beta = (dev(c[k]) for k in ("center", "mean", "rstd", "gamma", "beta"))
    for kind, place in (("contiguous", dev), ("slice", in_slice)):
        x, dy = place(c["x"], x_dt), place(c["dy"], dy_dt)
        assert (x.stride(0) > C) == (kind == "slice")
        for centred in (False, True):
            same(ops.bn_sums(x, center if centred else None), D.exact_bn_sums(c, centred, True)[0], "bn_sums %s centred=%s" % (kind, centred))
        for relu in (True, False):
            same(ops.bn_bwd_sums(dy, x, mean, rstd, gamma, beta, relu=relu), D.exact_bn_sums(c, False, relu)[1], "bn_bwd_sums %s relu=%s" % (kind, relu))
    torch.cuda.synchronize()
    ARENA.check()            # the guards of the (chunks, 2C) partial rows, the slices' neighbouring columns, the inputs


def bn_statistics(ops, x, rm=None, rv=None):
    """the engine's two-pass statistics: a first mean, then the sums centred on it"""
    C = x.shape[1]
    mean, rstd, center = e(C), e(C), e(C)
    ops.bn_finalize(ops.bn_sums(x), x.shape[0], None, None, center, rstd)
    ops.bn_finalize(ops.bn_sums(x, center), x.shape[0], rm, rv, mean, rstd, center=center)
    return mean, rstd


@pytest.mark.parametrize("C", D.BN_CHANNELS)
@pytest.mark.parametrize("rows", D.BN_ROWS)
def test_bn_apply_and_dx_at_chunk_seams_against_float64(ops, rows, C):
    c = D.bn_random_case(rows, C)
    x, dy, gam, bet = dev(c["x"]), dev(c["dy"]), dev(c["gamma"]), dev(c["beta"])
    mean, rstd = bn_statistics(ops, x)
    assert rel_err(mean.cpu(), c["mean"]) < D.TOL_FWD and rel_err(rstd.cpu(), (c["var"] + D.BN_EPS).rsqrt()) < D.TOL_FWD
    assert rel_err(ops.bn_apply(x, mean, rstd, gam, bet, e(rows, C)).cpu(), c["y"]) < D.TOL_FWD
    yb = ops.bn_apply(x, mean, rstd, gam, bet, out_slice(rows, C, BF16))
    assert rel_err(yb.float().cpu(), c["y"]) < D.TOL_BF16
    bs = ops.bn_bwd_sums(dy, x, mean, rstd, gam, bet)
    dx = ops.bn_bwd_dx(dy, x, mean, rstd, gam, bet, bs, rows, e(rows, C))
    far = (c["pre"].abs() > 1e-5).double()                                   # away from the ReLU's kink (tests/test_hip_uper_head.py)
    if rows >= D.SMALL_ROWS:
        assert rel_err(dx.cpu() * far, c["dx"] * far) < D.TOL_BWD
        assert rel_err(bs[:C].cpu(), c["dbeta"]) < D.TOL_BWD and rel_err(bs[C:].cpu(), c["dgamma"]) < D.TOL_BWD
        dxb = ops.bn_bwd_dx(dy, x, mean, rstd, gam, bet, bs, rows, out_slice(rows, C, BF16))
        assert rel_err(dxb.float().cpu() * far, c["dx"] * far) < D.TOL_BF16
    else:
        assert float(((dx.cpu().double() - c["dx"]) * far).abs().max()) < D.bn_dx_small_rows_bound(c["x"], c["gamma"], c["dy"])
    ARENA.check()


# ------------------------------------------------------------------------------------------------ B: regimes
@pytest.mark.parametrize("name,rows", D.REGIMES, ids=["%s-%d" % r for r in D.REGIMES])
def test_bn_regimes_within_the_restatements_bound(ops, name, rows):
    case = D.regime_case(name, rows)
    inp, ref, C = case["inp"], case["ref"], D.REGIME_C
    x, dy, gam, bet = dev(inp["x"]), dev(inp["dy"]), dev(inp["gamma"]), dev(inp["beta"])
    rm, rv = io(inp["rmean"]), io(inp["rvar"])
    mean, rstd = bn_statistics(ops, x, rm, rv)
    y = ops.bn_apply(x, mean, rstd, gam, bet, e(rows, C))
    bs = ops.bn_bwd_sums(dy, x, mean, rstd, gam, bet)
    dx = ops.bn_bwd_dx(dy, x, mean, rstd, gam, bet, bs, rows, e(rows, C))
    got = {k: v.cpu() for k, v in dict(mean=mean, rstd=rstd, rmean=rm, rvar=rv, y=y, dbeta=bs[:C], dgamma=bs[C:], dx=dx).items()}
    err = D.bn_errs(got, ref)
    for k in sorted(err):
        record_parity("decode", "bn_%s_%d_%s" % (name, rows, k), err[k])
        record_parity("decode", "bn_%s_%d_%s_restated_f32" % (name, rows, k), case["restated"][k])
        print("bn %s rows %d %-6s kernel %.3g  restated %.3g  bound %.3g" % (name, rows, k, err[k], case["restated"][k], case["bound"][k]))
    for k in sorted(err):
        assert err[k] <= case["bound"][k], (k, err[k], case["bound"][k])
    # the channel whose every pre-activation is negative: nothing comes through the ReLU, forward or backward, exactly
    assert float(got["y"][:, D.NEG_CH].abs().max()) == 0 and float(got["dx"][:, D.NEG_CH].abs().max()) == 0
    assert float(got["dbeta"][D.NEG_CH]) == 0 and float(got["dgamma"][D.NEG_CH]) == 0
    if name == "constant":       # variance 0: x - mean is exactly 0, so y is beta itself
        for ch in D.CONST_CH:
            assert torch.equal(got["y"][:, ch], inp["beta"][ch].expand(rows))
    if name == "one_row":
        assert float(got["dx"].abs().max()) == 0 and torch.equal(got["mean"], inp["x"][0])


# ------------------------------------------------------------------------------------------------ C: resize ratios
def rows_of(x):
    return D.to_rows(x).contiguous()


@pytest.mark.parametrize("along_w", [True, False], ids=["W", "H"])
@pytest.mark.parametrize("n_in", D.Z)
def test_resize_forward_and_backward_over_every_ratio(ops, n_in, along_w):
    """n_in -> every size of Z along one axis (2 -> 3 along the other), N = 1, C = 4: the forward; the backward's gather over lin_range with f32 dy, with
    bf16 dy, and accumulating onto dyadic presets -- against float64 F.interpolate and autograd"""
    C = D.RESIZE_C
    xd = dev(rows_of(D.resize_x(n_in, along_w)).float())
    for n_out in D.Z:
        c = D.resize_case(n_in, n_out, along_w)
        (Hi, Wi), (Ho, Wo) = D.grids(n_in, n_out, along_w)
        what = "%dx%d -> %dx%d" % (Hi, Wi, Ho, Wo)
        y = ops.resize_bilinear_fwd(xd, e(Ho * Wo, C), 1, Hi, Wi, Ho, Wo)
        assert rel_err(y.cpu(), rows_of(c["y"])) < D.TOL_FWD, what
        dyd = dev(rows_of(c["dy"]).float())
        dx = ops.resize_bilinear_bwd(dyd, e(Hi * Wi, C), 1, Hi, Wi, Ho, Wo)
        assert rel_err(dx.cpu(), rows_of(c["dx"])) < D.TOL_FWD, what
        acc = ops.resize_bilinear_bwd(dyd, io(rows_of(c["preset"]).float()), 1, Hi, Wi, Ho, Wo, accumulate=True)
        assert rel_err(acc.cpu(), rows_of(c["preset"] + c["dx"])) < D.TOL_FWD, what
        dxb = ops.resize_bilinear_bwd(in_slice(rows_of(c["dyb"]).float(), BF16), out_slice(Hi * Wi, C), 1, Hi, Wi, Ho, Wo)
        assert rel_err(dxb.cpu(), rows_of(c["dxb"])) < D.TOL_FWD, what + " (bf16 dy)"
    torch.cuda.synchronize()
    ARENA.check()


@pytest.mark.parametrize("n_in,n_out", D.BF16_FWD_PAIRS)
def test_resize_forward_into_a_bf16_column_slice(ops, n_in, n_out):
    for along_w in (True, False):
        c = D.resize_case(n_in, n_out, along_w)
        (Hi, Wi), (Ho, Wo) = D.grids(n_in, n_out, along_w)
        y = ops.resize_bilinear_fwd(dev(rows_of(c["x"]).float()), out_slice(Ho * Wo, D.RESIZE_C, BF16), 1, Hi, Wi, Ho, Wo)
        assert rel_err(y.float().cpu(), rows_of(c["y"])) < D.TOL_BF16
    ARENA.check()


def run_seg_ce(ops, logits, labels, K, N, h, w, dtype=F32, label_dtype=torch.uint8, ignore_index=255, loss_weight=0.7, ld=None):
    """-> (loss, dlogits (N h w, ld)) on the CPU.  The logits' pad columns hold NaN; logits and labels are frozen"""
    lr = dev(D.logit_rows(logits, K, ld), dtype)
    lab = dev(labels.to(label_dtype))
    loss, dl = ops.seg_ce(lr, K, N, h, w, lab, ignore_index, loss_weight)
    assert dl.shape == lr.shape and dl.dtype == F32
    return loss.cpu(), dl.cpu()


@pytest.mark.parametrize("along_w", [True, False], ids=["W", "H"])
@pytest.mark.parametrize("n", D.Z)
def test_seg_loss_gather_over_label_sizes_on_both_sides_of_the_logits(ops, n, along_w):
    """resize_bwd1_kernel is reachable only through seg_ce: K = 3 classes in a pitch of 8, logits of size n, labels finer and coarser than them"""
    K = D.SEG_K
    for m in D.seg_label_sizes(n):
        c = D.seg_ratio_case(n, m, along_w)
        loss, dl = run_seg_ce(ops, c["logits"], c["labels"], K, 1, c["h"], c["w"])
        what = "logits %dx%d, labels %dx%d" % (c["h"], c["w"], c["H"], c["W"])
        assert abs(loss.item() - c["loss"].item()) < D.TOL_LOSS * abs(c["loss"].item()), what
        assert rel_err(dl[:, :K], rows_of(c["dlogits"])) < D.TOL_DLOGITS, what
        assert float(dl[:, K:].abs().max()) == 0, what
    torch.cuda.synchronize()
    ARENA.check()


# ------------------------------------------------------------------------------------------------ D: the loss's regimes and instantiations
@pytest.mark.parametrize("name", D.SEG_CASES)
def test_seg_loss_regimes(ops, name):
    """float64 from the logits as the kernel's dtype holds them; 1e-5 on the loss, 1e-4 on the gradient (the kernel computes in f32 either way); a
    reference of exactly 0 (one class; every pixel ignored) must come back as exactly 0.  Pad columns: NaN going in, zero coming out."""
    c = D.seg_case(name)
    K = c["K"]
    loss, dl = run_seg_ce(ops, c["logits"], c["labels"], K, c["N"], c["h"], c["w"], c["dtype"], c["label_dtype"], c["ignore_index"], c["loss_weight"])
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dl).all())
    ref, dref = c["loss"].item(), rows_of(c["dlogits"])
    print("seg_ce %s: loss %.9g ref %.9g; dlogits rel err %.3g" % (name, loss.item(), ref, rel_err(dl[:, :K], dref) if float(dref.abs().max()) else 0.0))
    if ref == 0.0:
        assert loss.item() == 0.0 and float(dl.abs().max()) == 0.0
    else:
        assert abs(loss.item() - ref) < D.TOL_LOSS * abs(ref)
        assert rel_err(dl[:, :K], dref) < D.TOL_DLOGITS
    assert dl.shape[1] == D.pad8(K) and (dl.shape[1] == K or float(dl[:, K:].abs().max()) == 0)
    ARENA.check()


def test_seg_loss_refuses_4097_classes_and_writes_nothing(ops, monkeypatch):
    K = D.SEG_K_MAX + 1
    lr, lab = dev(torch.zeros(2, K)), dev(torch.zeros(1, 2, 2, dtype=torch.int64))          # pitch = K: the wrapper does not zero the gradient buffer first
    seen = watch_scratch(monkeypatch, ops)
    with pytest.raises(RuntimeError, match=D.ERR_ARG_TEXT % "mtp_seg_ce"):
        ops.seg_ce(lr, K, 1, 1, 2, lab)
    torch.cuda.synchronize()
    assert len(seen) == 3 and sorted(t.numel() for t in seen) == [1, 2 * K, 4 * K + 1] and all(still_poison(t) for t in seen)      # loss, dlogits, workspace


# ------------------------------------------------------------------------------------------------ E: channel_scale
@pytest.mark.parametrize("x_dt,y_dt", D.CS_DTYPES, ids=["f32", "bf16", "f32-bf16"])
@pytest.mark.parametrize("C", D.CS_C)
@pytest.mark.parametrize("rps", D.CS_RPS)
def test_channel_scale_is_bit_equal_to_torch(ops, rps, C, x_dt, y_dt):
    """Dropout2d: row r takes the mask row r / rows_per_sample.  Products with 0 and 2.0 are exact: contiguous, between column slices, and in place"""
    x, mask, ref = D.channel_scale_case(rps, C)
    md, rows = dev(mask), x.shape[0]
    same(ops.channel_scale(dev(x, x_dt), md, rps, e(rows, C, dtype=y_dt)), ref.double(), "contiguous")
    same(ops.channel_scale(in_slice(x, x_dt), md, rps, out_slice(rows, C, y_dt)), ref.double(), "slices")
    if x_dt == y_dt:             # the engine's use: y is x
        for buf in (io(x, x_dt), out_slice(rows, C, x_dt)):
            buf.copy_(x)
            out = ops.channel_scale(buf, md, rps, buf)
            assert out.data_ptr() == buf.data_ptr()
            same(buf, ref.double(), "in place")
    ARENA.check()


# ------------------------------------------------------------------------------------------------ F: tiles
def _fuse_input(shape, dt, g, offset):
    """the NCHW input on the device, frozen; offset: a contiguous view one element into its storage (its base is 4 or 2 bytes off a 16-byte boundary)"""
    f = D.pair_input(shape, dt, g)
    if not offset:
        return f, dev(f)
    flat = ARENA.like(torch.cat([f.new_zeros(1), f.reshape(-1)]))
    ARENA.frozen(flat)
    fd = flat[1:].view(shape)
    assert fd.is_contiguous() and fd.data_ptr() % 16 != 0
    return f, fd


FUSE_ALL = [(s, False) for s in D.FUSE_SHAPES] + [(D.FUSE_OFFSET_SHAPE, True)]
FUSE_IDS = ["x".join(map(str, s)) + ("-offset" if o else "") for s, o in FUSE_ALL]


@pytest.mark.parametrize("policy", D.FUSE_POLICIES)
@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (F32, BF16)], ids=["f32", "bf16", "f32-bf16"])
@pytest.mark.parametrize("shape,offset", FUSE_ALL, ids=FUSE_IDS)
def test_fuse_pair_forward_partial_tiles_are_bit_equal_to_torch(ops, shape, offset, in_dt, out_dt, policy):
    B, C, H, W = shape
    N = B // 2
    f, fd = _fuse_input(shape, in_dt, torch.Generator().manual_seed(C + H), offset)
    ref = D.to_rows(D.torch_fuse(f[:N], f[N:], policy)).to(out_dt)
    out = ops.fuse_pair_fwd(fd, out_slice(N * H * W, ref.shape[1], out_dt), policy)
    assert torch.equal(out.cpu(), ref)
    if offset:                   # the scalar kernel gives the bits of the vector kernel on the same values
        assert torch.equal(ops.fuse_pair_fwd(dev(f), e(N * H * W, ref.shape[1], dtype=out_dt), policy), out)
    ARENA.check()


@pytest.mark.parametrize("policy", D.FUSE_POLICIES)
@pytest.mark.parametrize("in_dt", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,offset", FUSE_ALL, ids=FUSE_IDS)
def test_fuse_pair_backward_partial_tiles_are_bit_equal_to_autograd(ops, shape, offset, in_dt, policy):
    B, C, H, W = shape
    N = B // 2
    g = torch.Generator().manual_seed(C + W)
    f, fd = _fuse_input(shape, in_dt, g, offset)
    x = f.clone().requires_grad_(True)
    y = D.torch_fuse(x[:N], x[N:], policy)
    gr = D.dyadic(y.shape, g)
    y.backward(gr.to(in_dt))
    df = ops.fuse_pair_bwd(in_slice(D.to_rows(gr)), fd, e(B, C, H, W), policy)
    assert torch.equal(df.cpu(), x.grad.float())
    if policy == "abs_diff":
        eq = (f[:N] == f[N:])
        assert eq.any() and df.cpu()[:N][eq].abs().max() == 0 and df.cpu()[N:][eq].abs().max() == 0
    ARENA.check()


@pytest.mark.parametrize("dt", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cx,Cs", D.UP_CHANNELS)
@pytest.mark.parametrize("h,w,hs,ws", D.UP_CASES)
def test_up_cat_forward_with_a_skip_larger_than_the_output(ops, h, w, hs, ws, Cx, Cs, dt):
    N = 2
    g = torch.Generator().manual_seed(h * 7 + ws + Cx)
    x, sk = torch.randn(N, Cx, h, w, generator=g).to(dt), torch.randn(N, Cs, hs, ws, generator=g).to(dt)
    xd, sd = in_slice(D.to_rows(x)), in_slice(D.to_rows(sk))
    rows = N * 4 * h * w
    y = ops.unet_up_cat_fwd(xd, sd, out_slice(rows, Cx + Cs, dt), N, h, w, hs, ws)
    assert torch.equal(y[:, :Cx].cpu(), D.to_rows(F.interpolate(x.float(), scale_factor=2, mode="nearest")).to(dt))
    ref = ops.resize_bilinear_fwd(sd, out_slice(rows, Cx + Cs, dt)[:, Cx:], N, hs, ws, 2 * h, 2 * w)
    assert torch.equal(y[:, Cx:], ref)
    want = D.to_rows(F.interpolate(sk.double(), size=(2 * h, 2 * w), mode="bilinear", align_corners=False))
    assert rel_err(y[:, Cx:].float().cpu(), want) < (D.TOL_FWD if dt == F32 else D.TOL_BF16)
    if dt == F32:
        yb = ops.unet_up_cat_fwd(xd, sd, out_slice(rows, Cx + Cs, BF16), N, h, w, hs, ws)
        assert torch.equal(yb, y.to(BF16))
    ARENA.check()


@pytest.mark.parametrize("Cx,Cs", D.UP_CHANNELS)
@pytest.mark.parametrize("h,w,hs,ws", D.UP_CASES)
def test_up_cat_backward_with_a_skip_larger_than_the_output(ops, h, w, hs, ws, Cx, Cs):
    N = 2
    g = torch.Generator().manual_seed(h * 11 + ws + Cx)
    dy = D.dyadic((N, Cx + Cs, 2 * h, 2 * w), g)
    dyd = in_slice(D.to_rows(dy))
    x = torch.zeros(N, Cx, h, w, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(dy[:, :Cx])
    sk = torch.zeros(N, Cs, hs, ws, dtype=torch.float64, requires_grad=True)
    F.interpolate(sk, size=(2 * h, 2 * w), mode="bilinear", align_corners=False).backward(dy[:, Cx:].double())
    dx, dsk = ops.unet_up_cat_bwd(dyd, out_slice(N * h * w, Cx), out_slice(N * hs * ws, Cs), N, h, w, hs, ws)
    assert torch.equal(dx.cpu(), D.to_rows(x.grad))
    assert torch.equal(dsk, ops.resize_bilinear_bwd(dyd[:, Cx:], e(N * hs * ws, Cs), N, hs, ws, 2 * h, 2 * w))
    assert rel_err(dsk.cpu(), D.to_rows(sk.grad)) < D.TOL_FWD
    # accumulate adds onto preset values (dyadic: the sums of dx stay exact)
    px, ps = D.dyadic((N * h * w, Cx), g), D.dyadic((N * hs * ws, Cs), g)
    ax, asx = out_slice(N * h * w, Cx), out_slice(N * hs * ws, Cs)
    ax.copy_(px)
    asx.copy_(ps)
    ops.unet_up_cat_bwd(dyd, ax, asx, N, h, w, hs, ws, accumulate=True)
    assert torch.equal(ax.cpu(), px + D.to_rows(x.grad))
    assert torch.equal(asx, ops.resize_bilinear_bwd(dyd[:, Cx:], io(ps), N, hs, ws, 2 * h, 2 * w, accumulate=True))
    assert rel_err(asx.cpu(), ps.double() + D.to_rows(sk.grad)) < D.TOL_FWD
    ARENA.check()


@pytest.mark.parametrize("H,W,S", D.POOL_CASES)
def test_adaptive_pool_at_its_limit_of_64_bins(ops, H, W, S):
    N, C = 2, 8
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y_ref = F.adaptive_avg_pool2d(x, S)
    dy = torch.randn(y_ref.shape, generator=g).to(BF16).double()              # bf16 numbers: the same gradient for the f32 and the bf16 run
    y_ref.backward(dy)
    y = ops.adaptive_avg_pool_fwd(in_slice(rows_of(x.detach()).float()), e(N * S * S, C), N, H, W, S)
    assert rel_err(y.cpu(), rows_of(y_ref.detach())) < D.TOL_FWD
    want = rows_of(x.grad)
    for dt in DT:
        dyd = dev(rows_of(dy).float(), dt)
        dx = ops.adaptive_avg_pool_bwd(dyd, out_slice(N * H * W, C), N, H, W, S)
        assert rel_err(dx.cpu(), want) < D.TOL_FWD, DTN[dt]
        preset = D.dyadic((N * H * W, C), g)
        acc = out_slice(N * H * W, C)
        acc.copy_(preset)
        ops.adaptive_avg_pool_bwd(dyd, acc, N, H, W, S, accumulate=True)
        assert rel_err(acc.cpu(), preset.double() + want) < D.TOL_FWD, DTN[dt]
    ARENA.check()


def test_adaptive_pool_refuses_65_bins_and_writes_nothing(ops):
    N, C, H, W, S = 1, 8, 65, 63, D.POOL_S_MAX + 1
    x, dy = dev(torch.zeros(N * H * W, C)), dev(torch.zeros(N * S * S, C))
    y, dx = ARENA.wide(N * S * S, C), ARENA.wide(N * H * W, C)                 # no column registered: all of it must stay poison
    with pytest.raises(RuntimeError, match=D.ERR_ARG_TEXT % "mtp_adaptive_avg_pool_fwd"):
        ops.adaptive_avg_pool_fwd(x, y, N, H, W, S)
    with pytest.raises(RuntimeError, match=D.ERR_ARG_TEXT % "mtp_adaptive_avg_pool_bwd"):
        ops.adaptive_avg_pool_bwd(dy, dx, N, H, W, S)
    torch.cuda.synchronize()
    assert still_poison(y) and still_poison(dx)
    ARENA.check()
