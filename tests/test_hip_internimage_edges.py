"""GPU: the InternImage operators (csrc/dcnv3.hip, csrc/conv.hip) at their smallest and most ragged shapes and in adversarial sampling regimes, every
buffer out of the guard arena (tests/guard.py): outputs NaN-poisoned and between guards, inputs frozen, the wrappers' workspaces poisoned and guarded.
References are the same operation in float64 on the CPU, computed from the dtype-rounded inputs.  Every case first asserts, through the dispatch queries
(mtp_dcnv3_kernel / mtp_conv_kernel), the kernel it is there to exercise, and that the arena pointers it passes are 16-byte aligned.  Every output goes
through Arena.check_written before it is compared: the helpers within / close / same call it on whatever device tensor they are given.

DCNv3: every offset is a dyadic rational that bf16 holds exactly, so the sample positions are exact in f32 and identical on both sides; the bounds are
the project's (tests/test_hip_dcnv3.py): of the reference tensor's maximum, f32 1e-5 (grad_offset 2e-5), bf16 output 6e-3, f32 gradients of a bf16 call
2e-5; a reference that is identically zero is matched exactly.

Data movement (im2col3x3, conv3x3_pack / unpack, pack_rows_padded, cast_pad_rows, copy_rows) is compared with torch.equal.  The summing operators are held
to an element-wise bound that follows from the arithmetic: T f32 accumulations into an element, each product rounded once,

    |got - ref| <= 2 T 2^-24 sum|terms|   [+ 2^-8 |ref| for a bf16 output]

(the factor 2 covers the order of accumulation, the cross-block reduction of the partial sums and fused multiply-adds), with
    col2im3x3                 T = 10           9 taps + the accumulate addend
    dwconv3x3 fwd / dx        T = 10           9 taps + bias resp. the accumulate addend
    dwconv k x k fwd / dx     T = k^2 + 1
    dwconv3x3 / dwconv dw, db T = N H W        the pixel count
    scale_residual fwd / dz   T = 3            x + s gamma z: two products and an add
    scale_residual dgamma     T = rows + 2
softmax_groups (the kernel uses __expf) keeps the TOL table; center_feature_scale is held to TOL |ref| + 2^-23 sum|terms| per element: with a saturated
gate s and 1 - s each carry up to 2^-24 of ABSOLUTE error in f32 (1 - s cancels to 0 at logit +40), which a bound relative to a 1e-18 reference cannot grant.

tests/test_internimage_edges_host.py asserts on the CPU that the regimes are what their names say, that a float32 evaluation stays inside these
bounds with room to spare, and that the queries name these families without a device."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import guard
from conftest import rel_err
from oracle import dcnv3_oracle as D

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
DTID = ["f32", "bf16"]
TOL = {F32: 2e-4, BF16: 1.5e-2}
ARENA = None     # the running test's guard.Arena
ERR_ARG = r"^%s failed: invalid argument$"      # what _lib.check raises for MTP_ERR_ARG (-1) and for nothing else


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


def rnd(*shape, seed=0, scale=1.0, dtype=BF16):
    """normal values that `dtype` holds exactly (bf16 by default: the same inputs serve the f32 and the bf16 run)"""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape) + 7 * len(shape))) * scale
    return t.to(dtype).float()


def dev(t, dtype=None):
    """an op INPUT: guarded and frozen"""
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t, dtype=None):
    """updated in place by contract: guarded, not frozen"""
    return ARENA.like(t, dtype=dtype or t.dtype)


def e(*shape, dtype=F32):
    """an op OUTPUT: NaN-poisoned, between guards"""
    return ARENA.empty(*shape, dtype=dtype)


def aligned(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts if t is not None)


def written(t, what=""):
    """an arena output (or a registered column slice of one) carries no poison any more.  A column slice is handed over as a contiguous copy: check_written
    looks only at the bit pattern of the tensor it is given (it needs no arena record), and a same-dtype copy keeps the poison bits"""
    ARENA.check_written(t.contiguous() if not t.is_contiguous() else t, what or None)
    return t


def same(got, want, what=""):
    """a data-movement output: written in full and bit-identical to `want` (a CPU tensor of the same dtype)"""
    written(got, what)
    return torch.equal(got.cpu(), want)


def within(got, ref, bound, what=""):
    """element-wise |got - ref| <= bound, all in float64; a device output is first checked to be written in full (a host tensor is a reference evaluation)"""
    if got.is_cuda:
        written(got, what)
    got, ref = got.double().cpu().reshape(ref.shape), ref.double()
    err = (got - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), "%s: %d of %d elements outside the bound; worst |err| / bound = %.3g at %s" % (
        what, int((~ok).sum()), ok.numel(), float((err / bound.clamp_min(1e-300))[~ok].nan_to_num(float("inf")).max()), tuple((~ok).nonzero()[0].tolist()))


def sum_bound(T, mag, ref, out_dtype=F32):
    b = 2.0 * T * 2.0 ** -24 * mag.double()
    return b + 2.0 ** -8 * ref.double().abs() if out_dtype == BF16 else b


def close(got, ref, tol, what):
    """max error relative to the reference tensor's maximum below tol; a reference that is identically zero is matched exactly"""
    if got.is_cuda:
        written(got, what)
    got = got.double().cpu().reshape(ref.shape)
    if float(ref.abs().max()) == 0.0:
        assert bool((got == 0).all()), "%s: %d elements differ from an exactly-zero reference" % (what, int((got != 0).sum()))
    else:
        err = rel_err(got, ref)
        assert err < tol, "%s: %.3g of the maximum (bound %.1g)" % (what, err, tol)


# ================================================================================================ DCNv3
GRIDS = [(1, 1, 1, 1), (2, 1, 17, 1), (2, 17, 1, 2), (1, 2, 2, 1), (2, 15, 17, 2), (1, 16, 16, 3), (3, 17, 16, 1)]      # (N, H, W, G)
REGIMES = ["zero", "integer", "quarter", "reach", "outside", "one_hot_mask", "zero_mask"]
VARIANTS = [0, 4, 2]      # MTP_DCNV3_VARIANT: the window form / the 3 x 3 form where offset_scale is 1 or 2 / the per-corner scatter
DCN_TOL = {F32: dict(out=1e-5, grad_input=1e-5, grad_offset=2e-5, grad_mask=1e-5), BF16: dict(out=6e-3, grad_input=2e-5, grad_offset=2e-5, grad_mask=2e-5)}


def reach_of(os_):
    """launch_bwd: reach = ceil(half kernel span * |offset_scale|) + 1, half = 1 for 3 x 3"""
    return int(math.ceil(abs(os_))) + 1


def dcn_cases():
    """(regime, grid, offset_scale, group_channels, remove_center): every regime on every grid -- offset_scale 2 (InternImage's) and 1 alternate over the
    grids, `integer` runs with both, `reach` with 1, 2 and 0.5 (R = 2, 3, 2) -- and the three further geometries on the 15 x 17 grid"""
    out = []
    for gi, grid in enumerate(GRIDS):
        os_ = (2.0, 1.0)[gi % 2]
        for regime in REGIMES:
            if regime == "reach":
                out += [(regime, grid, s, 16, 0) for s in (1.0, 2.0, 0.5)]
            elif regime == "integer":
                out += [(regime, grid, s, 16, 0) for s in (1.0, 2.0)]
            else:
                out.append((regime, grid, os_, 16, 0))
    for regime in ("integer", "quarter"):
        out += [(regime, GRIDS[4], 2.0, 8, 0), (regime, GRIDS[4], 2.0, 4, 0), (regime, GRIDS[4], 2.0, 16, 1)]
    return out


def dcn_id(c):
    return "%s-%s-os%g-gc%d%s" % (c[0], "x".join(str(v) for v in c[1]), c[2], c[3], "-rmc" if c[4] else "")


def _choice(vals, shape, g):
    return torch.tensor(vals)[torch.randint(0, len(vals), shape, generator=g)]


@functools.lru_cache(maxsize=None)
def dcn_case(regime, grid, os_, GC=16, rmc=0):
    """CPU inputs of one case (float32 tensors holding bf16-exact values) and the float64 oracle's four results.  With e = offset_scale * offset (px) a
    sample sits at (output pixel) + (i - 1, j - 1) offset_scale + e."""
    N, H, W, G = grid
    P = 9 - rmc
    seed = sum(ord(ch) for ch in regime) + 131 * (N + 3 * H + 7 * W + 11 * G) + int(8 * os_) + GC + rmc
    g = torch.Generator().manual_seed(seed)
    pts = D._points(3, 3, rmc)
    pi = torch.tensor([p[0] - 1.0 for p in pts]).view(1, 1, 1, 1, P)
    pj = torch.tensor([p[1] - 1.0 for p in pts]).view(1, 1, 1, 1, P)
    sh = (N, H, W, G, P)
    ho, wo = torch.arange(H).float().view(1, H, 1, 1, 1), torch.arange(W).float().view(1, 1, W, 1, 1)
    ints = lambda: torch.randint(-3, 4, sh, generator=g).float()
    mask = torch.softmax(torch.randn(N, H, W, G, P, generator=g), -1).to(BF16).float()
    if regime == "zero":
        ex, ey = torch.zeros(sh), torch.zeros(sh)
    elif regime == "integer":
        ex, ey = ints(), ints()
        c = P // 2       # the centre point (i = j = 1): nominally on its own output pixel
        ex[0, 0, 0, 0, c] = -1.0                     # exactly -1
        ey[N - 1, H - 1, W - 1, G - 1, c] = 1.0      # exactly H
        ex[N - 1, H - 1, W - 1, G - 1, 3] = 1.0      # point (i = 1, j = 0): exactly W
    elif regime in ("quarter", "one_hot_mask", "zero_mask"):
        ex, ey = ints() + 0.25, ints() + 0.25
        if regime == "one_hot_mask":
            mask = F.one_hot(torch.randint(0, P, (N, H, W, G), generator=g), P).float()
        elif regime == "zero_mask":
            mask = torch.zeros(sh)
    elif regime == "reach":
        # half the samples: the total displacement d from the output pixel on the last position inside the window reach R (corners R - 1, R), on its border,
        # astride it (corner R + 1 goes through the atomics) and beyond; the other half the same around the 3 x 3 form's reach of one pixel about the nominal position
        R = float(reach_of(os_))
        dvals = [R - 0.5, R, R + 0.5, R + 1.5, -(R - 0.5), -R, -(R + 0.5), -(R + 1.5), 0.25]
        evals = [0.5, 1.0, 1.5, 2.5, -0.5, -1.0, -1.5, -2.5]
        win = torch.rand(sh, generator=g) < 0.5
        ex = torch.where(win, _choice(dvals, sh, g) - pi * os_, _choice(evals, sh, g))
        ey = torch.where(win, _choice(dvals, sh, g) - pj * os_, _choice(evals, sh, g))
    elif regime == "outside":
        # one axis more than a pixel outside (-2.5 or size + 1.5), the other anywhere
        side = torch.randint(0, 4, sh, generator=g)
        ex, ey = ints() + 0.25, ints() + 0.25
        ex = torch.where(side == 0, -2.5 - wo - pi * os_, torch.where(side == 1, W + 1.5 - wo - pi * os_, ex))
        ey = torch.where(side == 2, -2.5 - ho - pj * os_, torch.where(side == 3, H + 1.5 - ho - pj * os_, ey))
    else:
        raise KeyError(regime)
    off = (torch.stack([ex, ey], -1) / os_).reshape(N, H, W, G * P * 2)
    assert torch.equal(off.to(BF16).float(), off), "offsets must be exact in bf16"
    mask = mask.reshape(N, H, W, G * P)
    x, gout = rnd(N, H, W, G * GC, seed=seed), rnd(N, H, W, G * GC, seed=seed + 1)
    args = (3, 3, 1, 1, 1, 1, 1, 1, G, GC, os_)
    ref = dict(out=D.dcnv3_forward(x.double(), off.double(), mask.double(), *args, rmc))
    ref["grad_input"], ref["grad_offset"], ref["grad_mask"] = D.dcnv3_backward(x.double(), off.double(), mask.double(), *args, gout.double(), rmc)
    return dict(x=x, off=off, mask=mask, gout=gout, args=args, rmc=rmc, grid=grid, ref=ref)


def want_fwd(GC, rmc, variant):
    if GC % 8 == 0 and not rmc and not variant & 8:
        return "fwd9"
    return "fwd_vec8" if GC % 8 == 0 else "fwd_scalar"


def want_bwd(GC, os_, variant):
    if variant & 2 or GC != 16:
        return "bwd_scatter_shfl"
    if variant & 4 and os_ in (1.0, 2.0):
        return "bwd_3x3_os1" if os_ == 1.0 else "bwd_3x3_os2"
    return "bwd_window_r2" if reach_of(os_) <= 2 else "bwd_window_r3"


def dcn_forward(c, dtype, variant, monkeypatch, tensors=None):
    """the forward on arena buffers -> (inputs, output); the query is asserted first"""
    import ctypes as C
    from mtp_amd import _lib
    from mtp_amd.ops_dcnv3 import functions as Fn
    monkeypatch.setenv("MTP_DCNV3_VARIANT", str(variant))
    N, H, W, G = c["grid"]
    GC = c["args"][9]
    x, off, m, gout = tensors or tuple(dev(c[k], dtype) for k in ("x", "off", "mask", "gout"))
    y = e(N, H, W, G * GC, dtype=dtype)
    assert aligned(x, off, m, y)
    assert Fn.dcnv3_kernel(x, off, m, y, *c["args"], 256, c["rmc"]) == Fn.DCNV3_KERNEL[want_fwd(GC, c["rmc"], variant)]
    g = Fn._geom(x, *c["args"], 256, c["rmc"])
    _lib.check(Fn.lib().mtp_dcnv3_fwd(x.data_ptr(), off.data_ptr(), m.data_ptr(), y.data_ptr(), Fn._dt(x), C.byref(g), Fn._s()), "mtp_dcnv3_fwd")
    ARENA.check_written(y)
    return (x, off, m, gout), y


def dcn_backward(c, tensors, variant, monkeypatch):
    import ctypes as C
    from mtp_amd import _lib
    from mtp_amd.ops_dcnv3 import functions as Fn
    monkeypatch.setenv("MTP_DCNV3_VARIANT", str(variant))
    x, off, m, gout = tensors
    grads = [e(*t.shape) for t in (x, off, m)]
    assert aligned(x, off, m, gout, *grads)
    assert Fn.dcnv3_kernel(x, off, m, gout, *c["args"], 256, c["rmc"], grads=grads) == Fn.DCNV3_KERNEL[want_bwd(c["args"][9], c["args"][10], variant)]
    g = Fn._geom(x, *c["args"], 256, c["rmc"])
    _lib.check(Fn.lib().mtp_dcnv3_bwd(x.data_ptr(), off.data_ptr(), m.data_ptr(), gout.data_ptr(), Fn._dt(x), grads[0].data_ptr(), grads[1].data_ptr(),
                                      grads[2].data_ptr(), C.byref(g), Fn._s()), "mtp_dcnv3_bwd")
    for t in grads:
        ARENA.check_written(t)
    return grads


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("case", dcn_cases(), ids=dcn_id)
def test_dcnv3_sampling_regimes_against_the_float64_oracle(case, dtype, monkeypatch):
    """forward and the three backward variants (window form, 3 x 3 form, per-corner scatter), each against oracle/dcnv3_oracle.py in float64: maps below
    one 16 x 16 tile, tile seams at 15 / 16 / 17, samples on pixel centres, on exact integers including -1, H and W, on and around the border of the gather
    form's reach, all outside, one-hot and zero masks; group widths 8 and 4 (the generic forwards, the scatter backward) and remove_center"""
    regime, grid, os_, GC, rmc = case
    c = dcn_case(*case)
    what = dcn_id(case) + " " + DTID[DT.index(dtype)]
    tensors, y = dcn_forward(c, dtype, 0, monkeypatch)
    close(y, c["ref"]["out"], DCN_TOL[dtype]["out"], what + " out")
    if GC == 8:      # 3 x 3 with 8-channel groups takes the unrolled forward by default; the generic 8-channel kernel through its A/B switch
        _, y8 = dcn_forward(c, dtype, 8, monkeypatch, tensors)
        close(y8, c["ref"]["out"], DCN_TOL[dtype]["out"], what + " out (generic forward)")
    for variant in VARIANTS:
        for name, got in zip(("grad_input", "grad_offset", "grad_mask"), dcn_backward(c, tensors, variant, monkeypatch)):
            close(got, c["ref"][name], DCN_TOL[dtype][name], "%s variant %d %s" % (what, variant, name))


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("os_", [2.0, 1.0])
def test_dcnv3_image_0_does_not_depend_on_image_1(os_, dtype, monkeypatch):
    """two images that differ only in image 1: image 0's output, grad_offset and grad_mask (plain stores) are bit-identical to a one-image run, its
    grad_input (f32 atomics for the far samples: rounding order only) to 2e-6 -- the n indexing of the 16 x 16 tile decomposition, a map off the tile both ways
    (17 x 24 x 4 groups = 51 whole waves of 32 (pixel, group) items per image: image 0 takes the same write-out path of the offset / mask kernel in both runs)"""
    H, W, G, GC, P = 17, 24, 4, 16, 9
    one = {k: rnd(*s, seed=i, scale=sc) for i, (k, s, sc) in enumerate((("x", (1, H, W, G * GC), 1.0), ("off", (1, H, W, G * P * 2), 1.5), ("gout", (1, H, W, G * GC), 1.0)))}
    one["mask"] = torch.softmax(rnd(1, H, W, G, P, seed=5), -1).reshape(1, H, W, G * P).to(BF16).float()
    two = {k: torch.cat([v, rnd(*v.shape, seed=20 + i, scale=1.5) if k != "mask" else v.flip(1)]) for i, (k, v) in enumerate(one.items())}
    args = (3, 3, 1, 1, 1, 1, 1, 1, G, GC, os_)
    c1, c2 = dict(one, args=args, rmc=0, grid=(1, H, W, G)), dict(two, args=args, rmc=0, grid=(2, H, W, G))
    t1, y1 = dcn_forward(c1, dtype, 0, monkeypatch)
    t2, y2 = dcn_forward(c2, dtype, 0, monkeypatch)
    assert torch.equal(y2[:1], y1)
    for variant in VARIANTS:
        g1, g2 = dcn_backward(c1, t1, variant, monkeypatch), dcn_backward(c2, t2, variant, monkeypatch)
        assert torch.equal(g2[1][:1], g1[1]) and torch.equal(g2[2][:1], g1[2]), variant
        assert rel_err(g2[0][:1].cpu(), g1[0].cpu()) < 2e-6, variant


# ================================================================================================ conv.hip: depth-wise convolutions
# (N, H, W, C).  The weight gradient runs ceil(pixels / 128) <= 1024 pixel blocks of ceil4(ceil(pixels / blocks)) pixels: below the cap a block holds at most 128
# pixels and none can be empty (151 x 28 = 4228 pixels: 34 blocks of 128, the last one holds 4); blocks are empty only beyond 1024 x 128 pixels, where rounding
# the block up to whole 4-pixel groups frees the tail -- 363 x 364 = 132132 pixels: 1024 blocks of 132, the last 23 empty.  That shape is the last one.
DW3_SHAPES = [(3, 1, 8, 8), (2, 2, 8, 260), (2, 5, 16, 516), (1, 8, 4, 8), (2, 3, 12, 264), (1, 151, 28, 8), (2, 1, 1, 4), (1, 2, 3, 12), (1, 363, 364, 4)]


def dw3_empty_blocks(lib, N, H, W):
    """pixel blocks of the 4-pixel weight-gradient kernel that hold no pixel, from mtp_dwconv3x3_bwd_dw_partial_rows and the launcher's block size"""
    rows, nb = N * H * W, lib.mtp_dwconv3x3_bwd_dw_partial_rows(N, H, W)
    ppb4 = (-(-rows // nb) + 3) // 4 * 4
    return nb - -(-rows // ppb4)
DWK_SHAPES = [(2, 2, 3, 8), (1, 7, 7, 260)]
DWK_KS = [1, 5, 15]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def dwconv_eval(x, dy, w, b, k, dt):
    """(y, dx, dw, db) of the depth-wise k x k convolution, stride 1, "same" padding, channels-last, evaluated in dtype dt on the CPU"""
    N, H, W, Cc = x.shape
    x, dy, w, b = x.to(dt), dy.to(dt), w.to(dt), b.to(dt)
    conv = lambda t, ww: _nhwc(F.conv2d(_nchw(t), ww, None, padding=k // 2, groups=Cc))
    xp = F.pad(_nchw(x), (k // 2,) * 4)
    dw = torch.zeros(Cc, 1, k, k, dtype=dt)      # dw[c, i, j] = sum_pixels dy[h, w] x[h + i - p, w + j - p]
    for i in range(k):
        for j in range(k):
            dw[:, 0, i, j] = (_nchw(dy) * xp[:, :, i:i + H, j:j + W]).sum((0, 2, 3))
    return conv(x, w) + b, conv(dy, w.flip(2, 3)), dw, dy.sum((0, 1, 2))


@functools.lru_cache(maxsize=None)
def dwconv_case(N, H, W, Cc, k=3):
    """inputs (bf16-exact activations, f32 weights), float64 references and the sums of |terms| of the depth-wise k x k convolution and its gradients"""
    x, dy = rnd(N, H, W, Cc, seed=1), rnd(N, H, W, Cc, seed=2)
    w, b, base = rnd(Cc, 1, k, k, seed=3, scale=0.3, dtype=F32), rnd(Cc, seed=4, dtype=F32), rnd(N, H, W, Cc, seed=5, dtype=F32)
    y, dx, dw, db = dwconv_eval(x, dy, w, b, k, torch.float64)
    ymag, dxmag, dwmag, dbmag = dwconv_eval(x.abs(), dy.abs(), w.abs(), b.abs(), k, torch.float64)
    return dict(x=x, dy=dy, w=w, b=b, base=base, k=k, y=y, ymag=ymag, dx=dx, dxmag=dxmag, dw=dw, dwmag=dwmag, db=db, dbmag=dbmag)


def want_dw3(op, dtype, W):
    if op == "dwconv3x3_bwd_dw":
        return "px4" if dtype == BF16 and W % 4 == 0 else "element"
    return "p8" if dtype == BF16 and W % 8 == 0 else "element"


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("N,H,W,Cc", DW3_SHAPES)
def test_dwconv3x3_edge_shapes(ops, dtype, N, H, W, Cc):
    """image seams (N > 1), a second channel block (C / 4 > 64), W == 8 (one lane holds both padding columns), H == 1, pixel blocks that start mid-row, empty
    trailing pixel blocks; forward, data gradient (= and +=) and weight / bias gradient"""
    c = dwconv_case(N, H, W, Cc)
    rows, K = N * H * W, ops.CONV_KERNEL
    xa, dya, wa, ba = dev(c["x"].reshape(rows, Cc), dtype), dev(c["dy"].reshape(rows, Cc), dtype), dev(c["w"]), dev(c["b"])
    y = e(rows, Cc, dtype=dtype)
    assert aligned(xa, dya, wa, ba, y)
    assert ops.conv_kernel("dwconv3x3_fwd", xa, y, N, H, W, Cc, w=wa, b=ba) == K[want_dw3("dwconv3x3_fwd", dtype, W)]
    ops.dwconv3x3_fwd(xa, wa, ba, y, N, H, W)
    within(y, c["y"], sum_bound(10, c["ymag"], c["y"], dtype), "dwconv3x3_fwd")
    for acc in (False, True):
        dx = io(c["base"].reshape(rows, Cc)) if acc else e(rows, Cc)
        assert aligned(dx) and ops.conv_kernel("dwconv3x3_bwd_dx", dya, dx, N, H, W, Cc, w=wa) == K[want_dw3("dwconv3x3_bwd_dx", dtype, W)]
        ops.dwconv3x3_bwd_dx(dya, wa, dx, N, H, W, accumulate=acc)
        ref, mag = (c["dx"] + c["base"].double(), c["dxmag"] + c["base"].double().abs()) if acc else (c["dx"], c["dxmag"])
        within(dx, ref, sum_bound(10, mag, ref), "dwconv3x3_bwd_dx accumulate=%s" % acc)
    assert ops.conv_kernel("dwconv3x3_bwd_dw", dya, None, N, H, W, Cc) == K[want_dw3("dwconv3x3_bwd_dw", dtype, W)]
    if (N, H, W) == (1, 151, 28):      # blocks that start mid-row (128 is no multiple of 28), a last block of 4 pixels, none empty
        assert ops.lib().mtp_dwconv3x3_bwd_dw_partial_rows(N, H, W) == 34 and dw3_empty_blocks(ops.lib(), N, H, W) == 0
    if (N, H, W) == (1, 363, 364):     # empty trailing blocks: they must still write zero partials (the poisoned workspace would show in dw otherwise)
        assert dw3_empty_blocks(ops.lib(), N, H, W) >= 1
    dw, db = e(Cc, 1, 3, 3), e(Cc)
    ops.dwconv3x3_bwd_dw(dya, xa, dw, db, N, H, W)
    within(dw, c["dw"], sum_bound(rows, c["dwmag"], c["dw"]), "dwconv3x3_bwd_dw")
    within(db, c["db"], sum_bound(rows, c["dbmag"], c["db"]), "dwconv3x3_bwd_dw bias")


def test_dwconv3x3_weights_off_16_bytes_take_the_element_kernel(ops):
    """a weight tensor that starts 4 bytes past a 16-byte boundary: the 8-pixel kernel loads its weights as float4, so the dispatch must fall back"""
    N, H, W, Cc = 2, 2, 8, 260
    c = dwconv_case(N, H, W, Cc)
    rows = N * H * W
    big = dev(torch.cat([torch.zeros(1), c["w"].reshape(-1)]))
    w1 = big[1:].view(Cc, 1, 3, 3)
    xa, ba, y = dev(c["x"].reshape(rows, Cc), BF16), dev(c["b"]), e(rows, Cc, dtype=BF16)
    assert w1.data_ptr() % 16 == 4 and aligned(xa, ba, y)
    assert ops.conv_kernel("dwconv3x3_fwd", xa, y, N, H, W, Cc, w=w1, b=ba) == ops.CONV_KERNEL["element"]
    ops.dwconv3x3_fwd(xa, w1, ba, y, N, H, W)
    within(y, c["y"], sum_bound(10, c["ymag"], c["y"], BF16), "dwconv3x3_fwd, weights off 16 bytes")


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("k", DWK_KS)
@pytest.mark.parametrize("N,H,W,Cc", DWK_SHAPES)
def test_dwconv_kxk_edge_shapes(ops, dtype, N, H, W, Cc, k):
    """k = 1 (no neighbours), 5 and 15 (wider than either map: most taps outside) on a 2 x 3 map and on 7 x 7 with a second channel block"""
    c = dwconv_case(N, H, W, Cc, k)
    rows = N * H * W
    xa, dya, wa, ba = dev(c["x"].reshape(rows, Cc), dtype), dev(c["dy"].reshape(rows, Cc), dtype), dev(c["w"]), dev(c["b"])
    y = ops.dwconv_fwd(xa, wa, ba, e(rows, Cc, dtype=dtype), N, H, W, k)
    within(y, c["y"], sum_bound(k * k + 1, c["ymag"], c["y"], dtype), "dwconv_fwd k=%d" % k)
    dx = ops.dwconv_bwd_dx(dya, wa, e(rows, Cc), N, H, W, k)
    within(dx, c["dx"], sum_bound(k * k + 1, c["dxmag"], c["dx"]), "dwconv_bwd_dx k=%d" % k)
    dx = ops.dwconv_bwd_dx(dya, wa, io(c["base"].reshape(rows, Cc)), N, H, W, k, accumulate=True)
    within(dx, c["dx"] + c["base"].double(), sum_bound(k * k + 1, c["dxmag"] + c["base"].double().abs(), c["dx"]), "dwconv_bwd_dx += k=%d" % k)
    dw, db = ARENA.zeros(Cc, 1, k, k), ARENA.zeros(Cc)
    ops.dwconv_bwd_dw(dya, xa, dw, db, N, H, W, k)
    within(dw, c["dw"], sum_bound(rows, c["dwmag"], c["dw"]), "dwconv_bwd_dw k=%d" % k)
    within(db, c["db"], sum_bound(rows, c["dbmag"], c["db"]), "dwconv_bwd_dw bias k=%d" % k)


# ================================================================================================ conv.hip: the 3 x 3 gathers
I2C_SHAPES = [(2, 1, 1, 8, False), (2, 1, 5, 8, False), (1, 2, 2, 16, False), (2, 7, 9, 8, False), (1, 8, 8, 24, False), (2, 3, 4, 12, False), (1, 5, 2, 3, True)]      # (N, H, W, Cin, NCHW f32 source)


def pad8(n):
    return (n + 7) // 8 * 8


def gather3x3_eval(x, dcols, stride, Kp, dt):
    """(cols, dx): im2col3x3 of x (N, H, W, Cin) with zero pad columns, and col2im3x3 of dcols (N Ho Wo, Kp), evaluated in dtype dt on the CPU"""
    N, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = F.pad(x.to(dt), (0, 0, 1, 1, 1, 1))
    cols, dxp = torch.zeros(N, Ho, Wo, Kp, dtype=dt), torch.zeros(N, H + 2, W + 2, Cin, dtype=dt)
    d4 = dcols.to(dt).reshape(N, Ho, Wo, Kp)
    for kh in range(3):
        for kw in range(3):
            t = (kh * 3 + kw) * Cin
            hs, ws = slice(kh, kh + stride * (Ho - 1) + 1, stride), slice(kw, kw + stride * (Wo - 1) + 1, stride)
            cols[..., t:t + Cin] = xp[:, hs, ws]
            dxp[:, hs, ws] += d4[..., t:t + Cin]
    return cols.reshape(-1, Kp), dxp[:, 1:H + 1, 1:W + 1]


@functools.lru_cache(maxsize=None)
def i2c_case(N, H, W, Cin, stride, extra):
    """x (N, H, W, Cin), its float64 im2col columns (N Ho Wo, Kp) with zero pad columns, random dcols and the float64 col2im of them (+ sum |terms|)"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Kp = pad8(9 * Cin) + extra
    x, base = rnd(N, H, W, Cin, seed=1), rnd(N, H, W, Cin, seed=3, dtype=F32)
    dcols = rnd(N * Ho * Wo, Kp, seed=2)
    cols, dx = gather3x3_eval(x, dcols, stride, Kp, torch.float64)
    return dict(x=x, base=base, dcols=dcols, cols=cols, dx=dx, dxmag=gather3x3_eval(x, dcols.abs(), stride, Kp, torch.float64)[1], Ho=Ho, Wo=Wo, Kp=Kp, stride=stride)


def want_i2c(dtype, Cin, nchw):
    return "v8" if dtype == BF16 and Cin % 8 == 0 and not nchw else "element"


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,H,W,Cin,nchw", I2C_SHAPES)
def test_im2col3x3_and_col2im3x3_edge_shapes(ops, dtype, N, H, W, Cin, nchw, stride, extra):
    """maps of one and two pixels a side, stride 1 and 2, Kp = pad8(9 Cin) and one 8-column step more (the zero branch k >= 9 Cin of the 8-channel kernel);
    im2col bit for bit with zero pad columns; col2im ignores pad columns that hold NaN poison, = and +=, and where the 8-channel kernel runs its f32 sums
    equal the element-wise kernel's bit for bit (forced through a destination whose pixel pitch is no multiple of 8)"""
    c = i2c_case(N, H, W, Cin, stride, extra)
    Ho, Wo, Kp, K = c["Ho"], c["Wo"], c["Kp"], ops.CONV_KERNEL
    want = K[want_i2c(dtype, Cin, nchw)]
    if nchw:
        src, strides = dev(_nchw(c["x"]).contiguous()), (Cin * H * W, W, 1, H * W)
    else:
        src, strides = dev(c["x"], dtype), (H * W * Cin, W * Cin, Cin, 1)
    cols = e(N * Ho * Wo, Kp, dtype=dtype)
    assert aligned(src, cols) and ops.conv_kernel("im2col3x3", src, cols, N, H, W, Cin, strides, stride, Kp) == want
    ops.im2col3x3(src, strides, cols, N, H, W, Cin, stride)
    assert same(cols, c["cols"].to(dtype), "im2col3x3") and float(cols[:, 9 * Cin:].float().abs().sum()) == 0.0
    # col2im: the pad columns of dcols keep the arena's NaN poison
    dcols = ARENA.empty(N * Ho * Wo, Kp, dtype=dtype)
    dcols[:, :9 * Cin] = c["dcols"][:, :9 * Cin].to(dtype)
    ARENA.frozen(dcols)
    shape = (N, Cin, H, W) if nchw else (N, H, W, Cin)
    perm = (lambda t: _nchw(t).contiguous()) if nchw else (lambda t: t)
    back = (lambda t: _nhwc(t)) if nchw else (lambda t: t)
    got = {}
    for acc in (False, True):
        dx = io(perm(c["base"])) if acc else e(*shape)
        assert aligned(dcols, dx) and ops.conv_kernel("col2im3x3", dcols, dx, N, H, W, Cin, strides, stride, Kp) == want
        ops.col2im3x3(dcols, dx, strides, N, H, W, Cin, stride, accumulate=acc)
        ref, mag = (c["dx"] + c["base"].double(), c["dxmag"] + c["base"].double().abs()) if acc else (c["dx"], c["dxmag"])
        within(back(dx), ref, sum_bound(10, mag, ref), "col2im3x3 accumulate=%s" % acc)
        got[acc] = dx
    if want == K["v8"]:
        ldw = Cin + 4                                             # pixel pitch off 8 elements: the element-wise kernel
        st2 = (H * W * ldw, W * ldw, ldw, 1)
        for acc in (False, True):
            wide = ARENA.wide(N * H * W, ldw)
            dst = ARENA.cols(wide, 0, Cin)
            if acc:
                dst.copy_(c["base"].reshape(-1, Cin))
            assert ops.conv_kernel("col2im3x3", dcols, wide, N, H, W, Cin, st2, stride, Kp) == K["element"]
            ops.col2im3x3(dcols, wide, st2, N, H, W, Cin, stride, accumulate=acc)
            assert torch.equal(written(dst).reshape(N, H, W, Cin), got[acc]), "8-channel and element-wise col2im sums differ (accumulate=%s)" % acc


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("Cout,Cin,extra", [(1, 1, 0), (5, 3, 8), (8, 8, 0), (3, 12, 8)])
def test_conv3x3_pack_and_unpack_edge_shapes(ops, dtype, Cout, Cin, extra):
    Kp = pad8(9 * Cin) + extra
    w = rnd(Cout, Cin, 3, 3, seed=1, dtype=F32)
    ref = torch.zeros(Cout, Kp)
    ref[:, :9 * Cin] = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    w2, w2t = e(Cout, Kp, dtype=dtype), e(Kp, Cout, dtype=dtype)
    ops.conv3x3_pack(dev(w), w2, w2t)
    assert same(w2, ref.to(dtype), "conv3x3_pack w2") and same(w2t, ref.t().contiguous().to(dtype), "conv3x3_pack w2t")
    only = e(Kp, Cout, dtype=dtype)
    ops.conv3x3_pack(dev(w), None, only)
    assert same(only, ref.t().contiguous().to(dtype), "conv3x3_pack w2t alone")
    dw2 = ARENA.empty(Cout, Kp)                                   # pad columns keep their poison: unpack must not read them into the result
    dw2[:, :9 * Cin] = ref[:, :9 * Cin]
    assert same(ops.conv3x3_unpack_grad(ARENA.frozen(dw2), e(Cout, Cin, 3, 3)), w, "conv3x3_unpack_grad")


# ================================================================================================ conv.hip: row-wise operators
SMX_REGIMES = ["equal", "one_high", "all_low", "ulp_ramp"]


def softmax_logits(regime, rows, G, P, ld, seed=0):
    """(rows, ld) bf16-exact logits; the pad columns G P .. ld hold +100 (a kernel that read them would show it)"""
    lg = torch.full((rows, ld), 100.0)
    v = torch.zeros(rows, G, P)
    if regime == "equal":
        v += 1.5
    elif regime == "one_high":
        hot = torch.randint(0, P, (rows, G), generator=torch.Generator().manual_seed(seed + rows + G + P))
        v = 60.0 * F.one_hot(hot, P).float()
    elif regime == "all_low":
        v -= 80.0
    elif regime == "ulp_ramp":
        v += 30.0 + 0.125 * (torch.arange(P).float() - P // 2)      # one bf16 ulp in [16, 32) is 2^-3
    lg[:, :G * P] = v.reshape(rows, G * P)
    assert torch.equal(lg.to(BF16).float(), lg)
    return lg


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("G", [1, 3, 24])
@pytest.mark.parametrize("P", [8, 9, 25])
def test_softmax_groups_regimes(ops, dtype, rows, padded, G, P):
    """the compile-time instantiations for 8 and 9 points and the run-time one, unpadded and padded rows, tied / dominated / very negative / one-ulp-apart
    logits against float64 softmax of the same logits; each group's probabilities sum to 1; the backward from the stored probabilities, pad columns zero"""
    ld = G * P + (7 if padded else 0)
    for regime in SMX_REGIMES:
        lg = softmax_logits(regime, rows, G, P, ld)
        ref = torch.softmax(lg[:, :G * P].double().reshape(rows, G, P), -1)
        prob = ops.softmax_groups_fwd(dev(lg, dtype), e(rows, G * P, dtype=dtype), G, P)
        pq = written(prob, "softmax_groups_fwd").double().cpu().reshape(rows, G, P)
        assert rel_err(pq, ref) < TOL[dtype], regime
        assert float((pq.sum(-1) - 1).abs().max()) < TOL[dtype], regime
        dp = rnd(rows, G, P, seed=3, dtype=F32)
        want = pq * (dp.double() - (pq * dp.double()).sum(-1, keepdim=True))
        dl = ops.softmax_groups_bwd(prob, dev(dp.reshape(rows, G * P)), e(rows, ld, dtype=dtype), G, P)
        # relative to the terms p (|dp| + sum p |dp|), not to the result: with one dominating logit the result cancels to 1e-26 at the hot point
        mag = pq * (dp.double().abs() + (pq * dp.double().abs()).sum(-1, keepdim=True))
        within(dl[:, :G * P], want.reshape(rows, G * P), TOL[dtype] * mag.reshape(rows, G * P), "softmax_groups_bwd " + regime)
        assert not padded or float(dl[:, G * P:].float().abs().max()) == 0.0, regime
        ARENA.check_written(dl)


def cfs_case(rows, G, GC, ld, sign):
    """center_feature_scale with saturated gates: logits of +-40 (sign 0: alternating), float64 references and the sums of |terms|"""
    Cc = G * GC
    y, xp, dout = rnd(rows, Cc, seed=1), rnd(rows, Cc, seed=2), rnd(rows, Cc, seed=4)
    lg = torch.full((rows, G), 40.0) * (sign if sign else torch.where((torch.arange(rows)[:, None] + torch.arange(G)[None, :]) % 2 == 0, 1.0, -1.0))
    lpad = torch.full((rows, ld), 100.0)
    lpad[:, :G] = lg
    s = torch.sigmoid(lg.double())[:, :, None].expand(rows, G, GC).reshape(rows, Cc)
    yd, xd, dd = y.double(), xp.double(), dout.double()
    prod = (dd * (xd - yd)).reshape(rows, G, GC)
    sg = torch.sigmoid(lg.double())
    return dict(y=y, xp=xp, dout=dout, lpad=lpad, out=yd * (1 - s) + xd * s, outmag=yd.abs() + xd.abs(), dy=dd * (1 - s), dxp=dd * s, dmag=dd.abs(),
                dl=sg * (1 - sg) * prod.sum(-1), dlmag=prod.abs().sum(-1))


def cfs_bound(ref, mag, dtype):
    return TOL[dtype] * ref.double().abs() + 2.0 ** -23 * mag.double()


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("rows,G,GC,ld,sign", [(1, 1, 4, 1, 1), (1, 1, 4, 8, -1), (257, 3, 4, 8, 0)])
def test_center_feature_scale_saturated_gate(ops, dtype, rows, G, GC, ld, sign):
    c = cfs_case(rows, G, GC, ld, sign)
    Cc = G * GC
    ya, xa, la, da = dev(c["y"], dtype), dev(c["xp"], dtype), dev(c["lpad"], dtype), dev(c["dout"], dtype)
    out = ops.center_feature_scale_fwd(ya, xa, la, e(rows, Cc, dtype=dtype), G)
    within(out, c["out"], cfs_bound(c["out"], c["outmag"], dtype), "center_feature_scale_fwd")
    dy, dxp, dl = e(rows, Cc, dtype=dtype), e(rows, Cc), e(rows, ld, dtype=dtype)
    ops.center_feature_scale_bwd(da, ya, xa, la, dy, dxp, dl, G)
    within(dy, c["dy"], cfs_bound(c["dy"], c["dmag"], dtype), "center_feature_scale_bwd dy")
    within(dxp, c["dxp"], cfs_bound(c["dxp"], c["dmag"], dtype), "center_feature_scale_bwd dxp")
    within(dl[:, :G], c["dl"], cfs_bound(c["dl"], c["dlmag"], dtype), "center_feature_scale_bwd dlogits")
    assert ld == G or float(dl[:, G:].float().abs().max()) == 0.0
    ARENA.check_written(dl)


def scale_residual_case(rows, Cc, rps):
    x, z, do = rnd(rows, Cc, seed=1, dtype=F32), rnd(rows, Cc, seed=2), rnd(rows, Cc, seed=4, dtype=F32)
    gamma = 0.5 + 0.1 * rnd(Cc, seed=3, dtype=F32)
    s = torch.tensor([0.0, 1.25, 0.5])[torch.arange(-(-rows // rps)) % 3]      # the sample scales include 0 (a dropped path)
    srow = s.repeat_interleave(rps)[:rows, None].double()
    t = srow * gamma.double() * z.double()
    return dict(x=x, z=z, do=do, gamma=gamma, s=s, out=x.double() + t, outmag=x.double().abs() + t.abs(), dz=srow * gamma.double() * do.double(),
                dg=(srow * do.double() * z.double()).sum(0), dgmag=(srow * do.double() * z.double()).abs().sum(0))


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("rows,Cc,rps", [(1, 4, 1), (257, 4, 100), (130, 1028, 7)])
def test_scale_residual_edge_rows(ops, dtype, rows, Cc, rps):
    """one row; 257 rows of one channel quad; 130 x 1028 with 7 rows per sample: the sample seam falls inside a row block and the last channel block is partial"""
    c = scale_residual_case(rows, Cc, rps)
    za, ga, sa = dev(c["z"], dtype), dev(c["gamma"]), dev(c["s"])
    out, outa = e(rows, Cc), e(rows, Cc, dtype=dtype)
    ops.scale_residual_fwd(dev(c["x"]), za, ga, out, outa, sa, rps)
    within(out, c["out"], sum_bound(3, c["outmag"], c["out"]), "scale_residual_fwd")
    within(outa, c["out"], sum_bound(3, c["outmag"], c["out"], dtype), "scale_residual_fwd act copy")
    dg = e(Cc)
    dz = ops.scale_residual_bwd(dev(c["do"]), za, ga, e(rows, Cc, dtype=dtype), dg, sa, rps)
    within(dz, c["dz"], sum_bound(3, c["dz"].abs(), c["dz"], dtype), "scale_residual_bwd dz")
    within(dg, c["dg"], sum_bound(rows + 2, c["dgmag"], c["dg"]), "scale_residual_bwd dgamma")


@pytest.mark.parametrize("dtype", DT, ids=DTID)
@pytest.mark.parametrize("rows", [1, 7, 108])
@pytest.mark.parametrize("n", [1, 7, 108])
def test_copy_pack_and_cast_rows_edge_shapes(ops, dtype, rows, n):
    """copy_rows with src_ld != dst_ld into a wider destination (the columns beyond n keep their poison); cast_pad_rows into rows of pad8(n) + 8; pack_rows_padded
    (rows, n) -> (pad8(rows), n) and its transpose (108 -> 112: the mask head); pad regions exactly zero"""
    src = rnd(rows, n + 3, seed=1, dtype=dtype)
    for dst_ld in (n, n + 5):
        wide = ARENA.wide(rows, dst_ld, dtype=dtype)
        ARENA.cols(wide, 0, n)
        ops.copy_rows(dev(src, dtype), wide, n)
        assert same(wide[:, :n], src[:, :n].to(dtype), "copy_rows")
    f = rnd(rows, n, seed=2, dtype=F32)
    for ld in (n, pad8(n) + 8):
        dst = ops.cast_pad_rows(dev(f), e(rows, ld, dtype=dtype))
        assert same(dst, torch.cat([f, torch.zeros(rows, ld - n)], 1).to(dtype), "cast_pad_rows") and float(dst[:, n:].float().abs().sum()) == 0.0
    Rp = pad8(rows)
    ref = torch.zeros(Rp, n)
    ref[:rows] = f
    wp, wpt = e(Rp, n, dtype=dtype), e(n, Rp, dtype=dtype)
    ops.pack_rows_padded(dev(f), wp, wpt)
    assert same(wp, ref.to(dtype), "pack_rows_padded wp") and same(wpt, ref.t().contiguous().to(dtype), "pack_rows_padded wpt")
    assert float(wp[rows:].float().abs().sum()) == 0.0 and float(wpt[:, rows:].float().abs().sum()) == 0.0


# ================================================================================================ refusals
def test_internimage_ops_refuse_illegal_shapes_without_launching(ops):
    """C % 4 != 0, Kp < 9 Cin, ld < G P, P > 32, an even k and Rp < R come back as MTP_ERR_ARG from the host-side argument checks: nothing is launched,
    every output (no column registered: all of it must stay poison) is untouched"""
    out, out16 = ARENA.wide(1, 4096), ARENA.wide(1, 4096, dtype=BF16)

    def refused(name, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=ERR_ARG % name):
            fn(*a, **kw)
    x6, w6, b6 = dev(rnd(12, 6, dtype=F32)), dev(rnd(6, 1, 3, 3, dtype=F32)), dev(rnd(6, dtype=F32))                     # C = 6
    refused("mtp_dwconv3x3_fwd", ops.dwconv3x3_fwd, x6, w6, b6, out.view(-1)[:72].view(12, 6), 1, 3, 4)
    refused("mtp_dwconv3x3_bwd_dx", ops.dwconv3x3_bwd_dx, x6, w6, out.view(-1)[:72].view(12, 6), 1, 3, 4)
    refused("mtp_dwconv3x3_bwd_dw", ops.dwconv3x3_bwd_dw, x6, x6, out.view(-1)[:54].view(6, 1, 3, 3), out.view(-1)[64:70], 1, 3, 4)
    refused("mtp_dwconv_fwd", ops.dwconv_fwd, x6, w6, b6, out.view(-1)[:72].view(12, 6), 1, 3, 4, 3)
    refused("mtp_scale_residual_fwd", ops.scale_residual_fwd, x6, x6, b6, out.view(-1)[:72].view(12, 6))
    refused("mtp_scale_residual_bwd", ops.scale_residual_bwd, x6, x6, b6, out.view(-1)[:72].view(12, 6), out.view(-1)[128:134])
    x8, w8, b8 = dev(rnd(12, 8, dtype=F32)), dev(rnd(8, 1, 4, 4, dtype=F32)), dev(rnd(8, dtype=F32))                     # even k
    for k in (2, 4):
        refused("mtp_dwconv_fwd", ops.dwconv_fwd, x8, w8, b8, out.view(-1)[:96].view(12, 8), 1, 3, 4, k)
        refused("mtp_dwconv_bwd_dx", ops.dwconv_bwd_dx, x8, w8, out.view(-1)[:96].view(12, 8), 1, 3, 4, k)
        refused("mtp_dwconv_bwd_dw", ops.dwconv_bwd_dw, x8, x8, out.view(-1)[:128].view(8, 1, 4, 4), out.view(-1)[128:136], 1, 3, 4, k)
    # Kp < 9 Cin (Cin = 8: 72 columns needed, 64 given); im2col3x3's wrapper asserts this itself, so the C entry point is called directly
    src = dev(rnd(1, 2, 2, 8), BF16)
    cols = out16.view(-1)[:4 * 64].view(4, 64)
    rc = ops.lib().mtp_im2col3x3(src.data_ptr(), 1, 32, 16, 8, 1, cols.data_ptr(), 1, 1, 2, 2, 8, 1, 64, None)
    assert rc == -1
    assert ops.lib().mtp_conv_kernel(0, src.data_ptr(), 1, 32, 16, 8, 1, cols.data_ptr(), 1, None, None, 1, 2, 2, 8, 1, 64) == -1
    refused("mtp_col2im3x3", ops.col2im3x3, dev(rnd(4, 64), BF16), out.view(-1)[:32].view(1, 2, 2, 8), (32, 16, 8, 1), 1, 2, 2, 8, 1)
    refused("mtp_conv3x3_pack", ops.conv3x3_pack, dev(rnd(2, 8, 3, 3, dtype=F32)), out.view(-1)[:128].view(2, 64), None)
    refused("mtp_conv3x3_unpack_grad", ops.conv3x3_unpack_grad, dev(rnd(2, 64, dtype=F32)), out.view(-1)[:144].view(2, 8, 3, 3))
    # ld < G P; P > 32
    refused("mtp_softmax_groups_fwd", ops.softmax_groups_fwd, dev(rnd(4, 17, dtype=F32)), out.view(-1)[:72].view(4, 18), 2, 9)
    refused("mtp_softmax_groups_bwd", ops.softmax_groups_bwd, dev(rnd(4, 18, dtype=F32)), dev(rnd(4, 18, dtype=F32)), out.view(-1)[:68].view(4, 17), 2, 9)
    refused("mtp_softmax_groups_fwd", ops.softmax_groups_fwd, dev(rnd(4, 33, dtype=F32)), out.view(-1)[:132].view(4, 33), 1, 33)
    refused("mtp_softmax_groups_bwd", ops.softmax_groups_bwd, dev(rnd(4, 33, dtype=F32)), dev(rnd(4, 33, dtype=F32)), out.view(-1)[:132].view(4, 33), 1, 33)
    # Rp < R
    refused("mtp_pack_rows_padded", ops.pack_rows_padded, dev(rnd(9, 4, dtype=F32)), out.view(-1)[:32].view(8, 4), out.view(-1)[64:96].view(4, 8))
    torch.cuda.synchronize()
    ARENA.check()
