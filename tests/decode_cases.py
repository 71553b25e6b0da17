"""Case tables, inputs, float64 references and bounds of the decode-head kernels (csrc/decode_head.hip, csrc/unet_head.hip), shared by
tests/test_hip_decode_edges.py (GPU) and tests/test_decode_edges_host.py (CPU).  Plain torch / numpy on the CPU: no device, no fixtures.

A. BatchNorm chunk seams.  `chunking` restates how mtp_bn_stats / mtp_bn_bwd_stats cut the rows into partial chunks; `BN_ROWS` are the row counts named
   for a seam each.  `exact_bn_case`: integers for which every sum of the statistics kernels is exact in f32 in any order (`exact_bn_terms`: the terms,
   which the host test proves to sum to less than 2^24 in absolute value), so the kernels return the integer bit for bit.  `bn_random_case`: random
   inputs at the same row counts, the float64 reference by autograd.
B. BatchNorm regimes.  `bn_math` is ONE statement of the arithmetic, parametrised by dtype: in float64 the reference, in float32 the RESTATEMENT of the
   kernels (f32 sums of x - center, the finalize in double on those sums, (x - mean) * rstd * gamma + beta, the backward's two sums), from which

       bound(output) = max(the project's tolerance, 4 x error of the float32 restatement against float64)

   With one_pass=True the variance is E[x^2] - E[x]^2 from f32 sums: what the engine's two-pass centred path exists to avoid.
C. Resize.  `Z`, the sizes; `lin_index_np` / `lin_range_np`: numpy float32 restatements of resize_common.h:lin_index and decode_head.hip:lin_range, with
   and without the contraction of a * b - c into an fma (the build leaves contraction on), and with `inv` moved by ulps; `range_cover` enumerates one
   (in, out) pair.  `seg_label_sizes`: the label sizes the loss's scalar-channel gather is run at per logit size.
D. `seg_case`: the segmentation-loss cases by name.  E / F: the shapes of channel_scale, fuse_pair, up_cat and the pooling.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTN = {F32: "f32", BF16: "bf16"}
MARGIN = 4.0
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# the project's tolerances for these kernels (tests/test_hip_uper_head.py, tests/test_hip_edges.py): max error relative to the tensor's max
TOL_FWD, TOL_BWD, TOL_BF16 = 1e-5, 1e-4, 8e-3
TOL_LOSS, TOL_DLOGITS = 1e-5, 1e-4


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def dyadic(shape, g):
    """multiples of 1/8 in [-8, 8]: bf16 numbers; sums of a few of them, and twice one, are exact in f32"""
    return torch.randint(-64, 65, tuple(shape), generator=g).float() / 8


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------ A: the chunk rule
BN_PART_MAX, BN_CHUNK_MIN, BN_WAVES = 512, 64, 4


def partial_rows(rows):
    """decode_head.hip:bn_partial_rows"""
    return min((rows + BN_CHUNK_MIN - 1) // BN_CHUNK_MIN, BN_PART_MAX)


def chunking(rows, nb=None):
    """(chunks, chunk length, index of the ragged chunk or None, its rows, empty chunks) as mtp_bn_stats cuts `rows`: chunk = ceil(rows / nb), workgroup b
    takes rows [b * chunk, min(rows, (b + 1) * chunk))"""
    nb = partial_rows(rows) if nb is None else nb
    chunk = -(-rows // nb)
    full, rest = divmod(rows, chunk)
    return nb, chunk, (full if rest else None), rest, nb - full - (1 if rest else 0)


BN_ROWS = [3, 5, 2400, 32768, 32769, 33281]
BN_CHANNELS = [4, 260]
# what each row count is named for: (chunks, chunk, ragged index, ragged rows, empty chunks)
BN_CHUNKING = {3: (1, 3, None, 0, 0), 5: (1, 5, None, 0, 0), 2400: (38, 64, 37, 32, 0), 32768: (512, 64, None, 0, 0), 32769: (512, 65, 504, 9, 7),
               33281: (512, 66, 504, 17, 7)}
SLICE_PAD = 4           # a column slice: pad columns on each side of the payload (pitch = C + 8)


@functools.lru_cache(maxsize=None)
def exact_bn_case(rows, C):
    """x, dy: integers in [-2, 2]; center: integers in [-1, 1].  With mean = 0, rstd = 1, gamma = 1, beta = 0 the backward has xhat = x and the ReLU mask
    x > 0.  Every row differs from its neighbours, so a row read twice, skipped or added to another chunk is another integer."""
    g = torch.Generator().manual_seed(6151 * rows + C)
    c = dict(rows=rows, C=C, x=ints(g, -2, 2, rows, C), dy=ints(g, -2, 2, rows, C), center=ints(g, -1, 1, C))
    c["mean"], c["rstd"], c["gamma"], c["beta"] = torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)
    return c


def exact_bn_sums(c, center, relu):
    """float64 [sum (x - center) | sum (x - center)^2] and [sum dy' | sum dy' x] of an exact case"""
    x, dy = c["x"].double(), c["dy"].double()
    v = x - (c["center"].double() if center else 0.0)
    d = dy * (x > 0).double() if relu else dy
    return torch.cat([v.sum(0), (v * v).sum(0)]), torch.cat([d.sum(0), (d * x).sum(0)])


def exact_bn_terms(c):
    """(name, terms summed along the rows) of every sum the two statistics kernels form on an exact case"""
    x, dy, k = c["x"].double(), c["dy"].double(), c["center"].double()
    out = []
    for name, v in (("x", x), ("x - center", x - k)):
        out += [("sum " + name, v), ("sum (%s)^2" % name, v * v)]
    for name, d in (("dy", dy), ("dy relu'", dy * (x > 0).double())):
        out += [("sum " + name, d), ("sum %s x" % name, d * x)]
    return out


def bn_autograd(x, gamma, beta, dy, relu=True, dtype=F64):
    """(pre, y, dx, dgamma, dbeta) of ReLU(BatchNorm(x)) in training mode by autograd in `dtype`"""
    xr, gr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    xh = (xr - xr.mean(0)) * (xr.var(0, unbiased=False) + BN_EPS).rsqrt()
    pre = xh * gr + br
    y = F.relu(pre) if relu else pre
    y.backward(dy.to(dtype))
    return pre.detach(), y.detach(), xr.grad, gr.grad, br.grad


@functools.lru_cache(maxsize=None)
def bn_random_case(rows, C):
    g = torch.Generator().manual_seed(31 * rows + C)
    c = dict(rows=rows, C=C, x=torch.randn(rows, C, generator=g), gamma=1 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
             dy=torch.randn(rows, C, generator=g))
    # no pre-activation within KINK of 0: there an f32 forward may take the other side of the ReLU than float64 (tests/test_hip_uper_head.py), which at
    # 2400 rows moves EVERY gradient of the channel by dy / rows through the two sums.  beta of such a channel moves by 1e-4 until none is left.
    xh = (c["x"].double() - c["x"].double().mean(0)) * (c["x"].double().var(0, unbiased=False) + BN_EPS).rsqrt()
    for _ in range(100):
        near = ((xh * c["gamma"].double() + c["beta"].double()).abs() < KINK).any(0)
        if not bool(near.any()):
            break
        c["beta"][near] += 1e-4
    c["pre"], c["y"], c["dx"], c["dgamma"], c["dbeta"] = bn_autograd(c["x"], c["gamma"], c["beta"], c["dy"])
    c["mean"], c["var"] = c["x"].double().mean(0), c["x"].double().var(0, unbiased=False)
    return c


def bn_dx_small_rows_bound(x, gam, dy):
    """tests/test_hip_edges.py:bn_dx_small_rows_bound, the same argument at three and five rows: dx = gamma rstd (dy' - mean(dy') - xhat mean(dy' xhat))
    cancels far below its terms, so an f32 evaluation promises 1e-4 of the scale of the TERMS, gamma rstd |dy|, not of the cancelled result"""
    var = x.double().var(0, unbiased=False)
    return TOL_BWD * float((gam.double() * (var + BN_EPS).rsqrt() * dy.double().abs()).max())


KINK = 5e-6             # twenty times the f32 rounding of a pre-activation of a few units
SMALL_ROWS = 63       # below this the backward is held to bn_dx_small_rows_bound, as tests/test_hip_edges.py does


# ------------------------------------------------------------------------------------------------ B: the arithmetic, once
def bn_math(inp, dtype, relu=True, one_pass=False):
    """every output of bn_stats x 2 -> bn_finalize x 2 -> bn_apply -> bn_bwd_stats -> bn_bwd_dx on `inp`, computed in `dtype`.  float64: the reference.
    float32: the kernels restated -- sums in f32, the finalize in double ON those sums (bn_finalize_kernel), everything else in f32.
    one_pass: no centring; the sums of x and x^2 in `dtype`, and the variance from them in `dtype` as well."""
    x, g, b, dy = (inp[k].to(dtype) for k in ("x", "gamma", "beta", "dy"))
    n = x.shape[0]
    if one_pass:
        m = x.sum(0) / n
        var = ((x * x).sum(0) / n - m * m).clamp_min(0).double()
        m = m.double()
    else:
        c = (x.sum(0).double() / n).to(dtype)                                   # the first pass: a first mean, rounded to the kernels' type
        v = x - c
        d = v.sum(0).double() / n
        var = ((v * v).sum(0).double() / n - d * d).clamp_min(0)
        m = c.double() + d
    eps = float(np.float32(BN_EPS)) if dtype == F32 else BN_EPS                  # the kernel's eps is a float argument
    mean, rstd = m.to(dtype), (1.0 / torch.sqrt(var + eps)).to(dtype)
    out = dict(mean=mean, rstd=rstd)
    if "rmean" in inp:
        mom = torch.tensor(BN_MOMENTUM, dtype=F32).to(dtype)
        unb = var * n / (n - 1.0) if n > 1 else var
        out["rmean"] = (1 - mom) * inp["rmean"].to(dtype) + mom * m.to(F32).to(dtype)
        out["rvar"] = (1 - mom) * inp["rvar"].to(dtype) + mom * unb.to(F32).to(dtype)
    xh = (x - mean) * rstd
    pre = xh * g + b
    out["y"] = pre.clamp_min(0) if relu else pre
    dd = dy * (pre > 0).to(dtype) if relu else dy
    s, q = dd.sum(0), (dd * xh).sum(0)
    inv = torch.tensor(1.0 / n, dtype=F64).to(dtype)                              # (float)(1.0 / count)
    out["dbeta"], out["dgamma"] = s, q
    out["dx"] = g * rstd * (dd - s * inv - xh * q * inv)
    return {k: v.double() for k, v in out.items()}


REGIMES = [("mean_1e4", 2400), ("mean_1e4", 5), ("constant", 2400), ("constant", 5), ("negative", 2400), ("negative", 5), ("one_row", 1)]
REGIME_C = 8
NEG_CH, CONST_CH = 1, (0, 5)            # the channel whose pre-activations are all negative; the constant channels
CONSTANTS = (3.0, -0.5)
ONE_PASS_FACTOR = 10.0
FLOORS = dict(mean=TOL_FWD, rstd=TOL_FWD, rmean=TOL_FWD, rvar=TOL_FWD, y=TOL_FWD, dx=TOL_BWD, dgamma=TOL_BWD, dbeta=TOL_BWD)


def bn_errs(got, ref):
    """output -> error: the mean in units of the channel's standard deviation (what it does to xhat), everything else relative to the reference's max"""
    return {k: (float(((got[k].double() - ref[k]).abs() * ref["rstd"]).max()) if k == "mean" else rel_err(got[k], ref[k])) for k in got}


@functools.lru_cache(maxsize=None)
def regime_case(name, rows):
    """inputs, float64 reference, the restatement's errors and the bounds of one regime.  No pre-activation lies near the ReLU's kink: beta is +-8 |gamma|
    and |xhat| < sqrt(rows) -- below 8 for the five rows, and for 2400 normal draws -- so the f32 and the float64 forward mask the same elements and
    the regimes test the statistics, not the kink (section A runs mixed masks exactly)."""
    i = [r[0] for r in REGIMES].index(name)
    g = torch.Generator().manual_seed(1009 * i + rows)
    C = REGIME_C
    n = torch.randn(rows, C, generator=g)
    x = 1e4 + n if name == "mean_1e4" else n.clone()
    if name == "constant":
        for ch, v in zip(CONST_CH, CONSTANTS):
            x[:, ch] = v
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 8 * gamma.abs()
    beta[NEG_CH] = -8 * gamma[NEG_CH].abs()
    inp = dict(x=x.float(), gamma=gamma, beta=beta, dy=torch.randn(rows, C, generator=g), rmean=0.1 * torch.randn(C, generator=g),
               rvar=0.5 + torch.rand(C, generator=g))
    ref, rst = bn_math(inp, F64), bn_math(inp, F32)
    err = bn_errs(rst, ref)
    return dict(inp=inp, ref=ref, restated=err, bound={k: max(FLOORS[k], MARGIN * err[k]) for k in err}, name=name, rows=rows)


# ------------------------------------------------------------------------------------------------ C: resize
Z = [1, 2, 3, 5, 7, 16, 63, 64, 65, 127, 255, 256, 257, 513]
RESIZE_C = 4
BF16_FWD_PAIRS = [(1, 513), (513, 1), (255, 256), (256, 255), (63, 65), (7, 3)]      # the forward into a bf16 column slice
SEG_K = 3               # the loss's gather: K = 3 classes, pitch pad8(K) = 8


def seg_label_sizes(n):
    """label sizes for logits of size n: the ends of Z, the neighbours of n in Z, n itself (ratio 1), and 16 / 64"""
    i = Z.index(n)
    return sorted({Z[0], Z[-1], Z[max(i - 1, 0)], Z[min(i + 1, len(Z) - 1)], n, 16, 64})


def _f(v):
    return np.float32(v)


def _mulsub(a, b, c, fma):
    """a * b - c in f32; fma: contracted (the product unrounded: exact in float64, one rounding of the difference to f32 up to a double rounding)"""
    if fma:
        return (a.astype(np.float64) * b.astype(np.float64) - np.float64(c)).astype(np.float32)
    return (a * b).astype(np.float32) - _f(c)


def lin_index_np(n_in, n_out, fma=False, scale=None):
    """resize_common.h:lin_index for every output o: (i0, i1, w0, w1), float32 throughout"""
    scale = _f(n_in) / _f(n_out) if scale is None else scale
    o = np.arange(n_out, dtype=np.float32)
    src = _mulsub(np.full(n_out, scale, np.float32), o + _f(0.5), 0.5, fma)
    src = np.where(src < 0, _f(0), src).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (_f(1) - w1).astype(np.float32), w1


def lin_range_np(n_in, n_out, fma=False, inv_ulps=0, margin=1):
    """decode_head.hip:lin_range for every source i: (lo, hi) as the kernel uses them and (lo_raw, hi_raw) before the clamps.  inv_ulps: `inv` moved by that
    many ulps (a division that is not correctly rounded); margin: the kernel's is 1"""
    inv = _f(n_out) / _f(n_in)
    for _ in range(abs(inv_ulps)):
        inv = np.nextafter(inv, _f(np.inf if inv_ulps > 0 else -np.inf))
    i = np.arange(n_in, dtype=np.float32)
    inv_v = np.full(n_in, inv, np.float32)
    lo_raw = np.floor(_mulsub(i - _f(0.5), inv_v, 0.5, fma)).astype(np.int64) - margin
    hi_raw = np.ceil(_mulsub(i + _f(1.5), inv_v, 0.5, fma)).astype(np.int64) + margin
    lo, hi = np.maximum(lo_raw, 0), np.minimum(hi_raw, n_out - 1)
    hi[n_in - 1] = n_out - 1
    return lo, hi, lo_raw, hi_raw


def range_cover(n_in, n_out, fma=False, inv_ulps=0, margin=1):
    """(outputs with a non-zero weight for some source i that lie outside [lo(i), hi(i)], the smallest slack of the unclamped bounds over the pair)"""
    i0, i1, w0, w1 = lin_index_np(n_in, n_out, fma)
    lo, hi, lo_raw, hi_raw = lin_range_np(n_in, n_out, fma, inv_ulps, margin)
    o = np.arange(n_out)
    same = i0 == i1
    missed, slack = 0, 1 << 30
    for i, w in ((i0, np.where(same, w0 + w1, w0)), (i1, np.where(same, _f(0), w1))):
        live = w != 0
        missed += int(((o < lo[i]) | (o > hi[i]))[live].sum())
        if live.any():
            slack = min(slack, int((o - lo_raw[i])[live].min()), int((hi_raw[i] - o)[live].min()))
    return missed, slack


def resize_matrix(n_in, n_out, fma=False):
    """(n_out, n_in) float64 matrix of lin_index_np's f32 weights: the resize with the kernels' index arithmetic and exact sums"""
    i0, i1, w0, w1 = lin_index_np(n_in, n_out, fma)
    W = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(W, (o, i0), w0.astype(np.float64))
    np.add.at(W, (o, i1), w1.astype(np.float64))
    return torch.from_numpy(W)


RESIZE_DECAY = 8.0


def _signed(g, *shape):
    """+-[0.5, 1.5]"""
    return ((0.5 + torch.rand(*shape, generator=g)) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).double()


def _decaying(g, C, n_other, pos):
    """(1, C, n_other, len(pos)) values +-[0.5, 1.5] / (1 + pos / 8): the gradient of the resize tests, its amplitude falling off along the resized axis"""
    return _signed(g, 1, C, n_other, len(pos)) / (1 + pos.double() / RESIZE_DECAY)


@functools.lru_cache(maxsize=None)
def resize_x(n_in, along_w):
    """the source of one size: (1, C, 2, n) or (1, C, n, 2) float64 holding f32 values, a cos(phi + 4 log(1 + i / 4)) per channel and line.
    The f32 index rule places a source position within a few 2^-24 of its own size (the rounding of in / out, of its product with the output index, of
    the position): up to 4e-5 at 512, more than the 1e-5 the resize is held to if neighbouring values differed by the tensor's max there.  Here the
    values keep their size along the axis but neighbours differ by 4 / (4 + i) of it, so that error stays near 1e-6 of the tensor's max whatever the
    ratio (tests/test_decode_edges_host.py measures it on these very inputs), while an index off by one (0.8 % of the max at 512) or a dropped
    contribution is hundreds of times the tolerance.  The gradients decay in amplitude instead (_decaying)."""
    g = torch.Generator().manual_seed(n_in * 2 + along_w)
    i = torch.arange(n_in).double()
    x = _signed(g, 1, RESIZE_C, 2, 1) * torch.cos(6.283 * torch.rand(1, RESIZE_C, 2, 1, generator=g).double() + 4 * torch.log1p(i / 4))
    x = x.float().double()
    return x if along_w else x.transpose(2, 3).contiguous()


@functools.lru_cache(maxsize=None)
def resize_case(n_in, n_out, along_w):
    """x, dy (f32 values), dyb (bf16 values), preset (dyadic) and the float64 F.interpolate / autograd results y, dx, dxb"""
    g = torch.Generator().manual_seed(n_in * 1031 + n_out * 2 + along_w)
    (Hi, Wi), (Ho, Wo) = grids(n_in, n_out, along_w)
    x = resize_x(n_in, along_w)
    dy = _decaying(g, RESIZE_C, 3, torch.arange(n_out) * (n_in / n_out)).float().double()
    dy = dy if along_w else dy.transpose(2, 3).contiguous()
    out = dict(x=x, dy=dy, dyb=dy.to(BF16).double(), preset=dyadic((1, RESIZE_C, Hi, Wi), g).double())
    for k, d in (("dx", out["dy"]), ("dxb", out["dyb"])):
        xr = x.clone().requires_grad_(True)
        y = F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=False)
        y.backward(d)
        out["y"], out[k] = y.detach(), xr.grad
    return out


def resize_restated(n_in, n_out, along_w, fma):
    """(y, dx) of resize_case with the f32 index arithmetic and float64 sums"""
    c = resize_case(n_in, n_out, along_w)
    Wa, Wb = resize_matrix(n_in, n_out, fma), resize_matrix(2, 3, fma)
    Wy, Wx = (Wb, Wa) if along_w else (Wa, Wb)
    return torch.einsum("oh,nchw,pw->ncop", Wy, c["x"], Wx), torch.einsum("oh,ncop,pw->nchw", Wy, c["dy"], Wx)


@functools.lru_cache(maxsize=None)
def seg_ratio_case(n, m, along_w):
    """the loss with logits (1, 3, 2, n) and labels (1, 3, m) (or transposed): logits, labels (uint8 values, a fifth ignored), loss, dlogits"""
    g = torch.Generator().manual_seed(n * 1201 + m * 2 + along_w)
    (h, w), (H, W) = grids(n, m, along_w)
    logits = torch.randn(1, SEG_K, h, w, generator=g)
    labels = torch.randint(0, SEG_K, (1, H, W), generator=g)
    labels[torch.rand(1, H, W, generator=g) < 0.2] = 255
    labels[0, 0, 0] = 1
    loss, dl = seg_loss_ref(logits, labels, 255, 0.7)
    return dict(logits=logits, labels=labels, loss=loss, dlogits=dl, h=h, w=w, H=H, W=W)


def seg_ratio_restated(n, m, along_w, fma):
    """(loss, dlogits) of seg_ratio_case with the f32 index arithmetic, everything else float64"""
    c = seg_ratio_case(n, m, along_w)
    Wa, Wb = resize_matrix(n, m, fma), resize_matrix(2, 3, fma)
    Wy, Wx = (Wb, Wa) if along_w else (Wa, Wb)
    lg = c["logits"].double().clone().requires_grad_(True)
    up = torch.einsum("oh,nchw,pw->ncop", Wy, lg, Wx)
    loss = 0.7 * F.cross_entropy(up, c["labels"], ignore_index=255, reduction="sum") / c["labels"].numel()
    loss.backward()
    return loss.detach(), lg.grad


def grids(n_in, n_out, along_w):
    """((Hi, Wi), (Ho, Wo)): n_in -> n_out along one axis, 2 -> 3 along the other"""
    return ((2, n_in), (3, n_out)) if along_w else ((n_in, 2), (n_out, 3))


# ------------------------------------------------------------------------------------------------ D: the segmentation loss
SEG_K_MAX = 4096
SEG_CASES = ["bf16_u8", "bf16_i64", "one_hot", "near_ties", "k1", "k4096", "ignore_neg100", "all_ignored", "many_partials", "ragged", "coarse_labels"]


def seg_loss_ref(logits, labels, ignore_index, loss_weight):
    """BaseDecodeHead.loss_by_feat in float64 (tests/test_uper_head.py:torch_seg_loss): (loss, d loss / d logits)"""
    lg = logits.double().clone().requires_grad_(True)
    up = F.interpolate(lg, size=labels.shape[1:], mode="bilinear", align_corners=False)
    loss = loss_weight * F.cross_entropy(up, labels.long(), ignore_index=ignore_index, reduction="sum") / labels.numel()
    loss.backward()
    return loss.detach(), lg.grad


@functools.lru_cache(maxsize=None)
def seg_case(name):
    """dict(logits (N, K, h, w) f32 holding values of `dtype`, labels (N, H, W) int64, label_dtype, dtype, ignore_index, loss, dlogits)"""
    g = torch.Generator().manual_seed(SEG_CASES.index(name) + 77)
    N, K, h, w, H, W, dtype, ldt, ign, frac, scale = 2, 5, 6, 7, 13, 9, F32, torch.uint8, 255, 0.2, 1.0
    if name in ("bf16_u8", "bf16_i64"):
        dtype, ldt, scale = BF16, (torch.uint8 if name == "bf16_u8" else torch.int64), 3.0
    elif name in ("one_hot", "near_ties"):
        h, w, ldt = H, W, torch.int64                    # ratio 1: the interpolation is the identity, so the logits the softmax sees are exact
    elif name == "k1":
        K = 1
    elif name == "k4096":
        N, K, h, w, H, W, frac, ldt = 1, SEG_K_MAX, 1, 2, 2, 2, 0.0, torch.int64          # (uint8 labels cannot name 4096 classes)
    elif name in ("ignore_neg100", "all_ignored"):
        ign, ldt = -100, torch.int64
    elif name == "many_partials":
        N, K, h, w, H, W = 1, 2, 65, 63, 257, 257       # 66049 pixels: 259 partials, sum_scale_kernel's second trip
    elif name == "ragged":
        N, K, h, w, H, W = 1, 19, 2, 3, 3, 7            # 21 pixels: one workgroup, 235 idle threads
    elif name == "coarse_labels":
        N, K, h, w, H, W = 2, 3, 16, 10, 5, 7           # labels coarser than the logits, no integer ratio
    logits = scale * torch.randn(N, K, h, w, generator=g)
    labels = torch.randint(0, K, (N, H, W), generator=g)
    if name == "one_hot":           # +-3e4: the label's class wins (loss 0) at most pixels, another class wins (loss 6e4) at every seventh
        win = torch.where(torch.arange(N * H * W).view(N, H, W) % 7 == 3, (labels + 1) % K, labels)
        logits = torch.full((N, K, h, w), -3e4).scatter_(1, win[:, None], 3e4)
    elif name == "near_ties":       # all classes within a few ulps (2^-9) to a few units of 3e4 or of -3e4
        base = torch.where(torch.rand(N, 1, h, w, generator=g) < 0.5, 3e4, -3e4)
        step = torch.tensor([0.0, 2.0 ** -9, 2.0 ** -8, 0.5, 2.0])[torch.randint(0, 5, (N, K, h, w), generator=g)]
        logits = base - step
    logits = logits.to(dtype).float()
    labels[torch.rand(N, H, W, generator=g) < frac] = ign
    if name == "all_ignored":
        labels[:] = ign
    elif frac:
        labels[0, 0, 0], labels[-1, -1, -1] = 0, ign
    loss, dl = seg_loss_ref(logits, labels, ign, 0.7)
    return dict(name=name, N=N, K=K, h=h, w=w, H=H, W=W, dtype=dtype, label_dtype=ldt, ignore_index=ign, logits=logits, labels=labels, loss=loss, dlogits=dl,
                loss_weight=0.7)


def pad8(n):
    return (n + 7) // 8 * 8


def logit_rows(logits, K=None, ld=None):
    """(N, K, h, w) -> (N h w, ld) rows whose pad columns hold NaN: the kernel must not read them"""
    K = logits.shape[1] if K is None else K
    ld = pad8(K) if ld is None else ld
    r = torch.full((logits.shape[0] * logits.shape[2] * logits.shape[3], ld), float("nan"))
    r[:, :K] = logits.permute(0, 2, 3, 1).reshape(-1, K)
    return r


# ------------------------------------------------------------------------------------------------ E: channel_scale
CS_N, CS_RPS, CS_C = 3, [1, 5, 64, 65], [4, 260]
CS_DTYPES = [(F32, F32), (BF16, BF16), (F32, BF16)]


def channel_scale_case(rps, C):
    """x dyadic, a mask of 0 and 2.0 whose three rows differ in every block of three channels: the product is exact, and a wrong mask row shows"""
    g = torch.Generator().manual_seed(rps * 1000 + C)
    x = dyadic((CS_N * rps, C), g)
    x[x == 0] = 0.125                                                            # no zeros: a dropped channel differs from a kept one everywhere
    mask = 2.0 * ((torch.arange(C)[None, :] + torch.arange(CS_N)[:, None]) % 3 != 0).float()
    ref = (x.view(CS_N, rps, C) * mask[:, None, :]).reshape(-1, C)
    return x, mask, ref


# ------------------------------------------------------------------------------------------------ F: tiles
FUSE_TILE = 64
# (2N, C, H, W), what it is there for
FUSE_SHAPES = [(2, 68, 2, 34), (2, 132, 5, 13), (2, 4, 8, 8), (6, 8, 1, 4)]
FUSE_OFFSET_SHAPE = (2, 8, 4, 4)        # read through a view one element into its storage: the base fails the 16-byte test
FUSE_POLICIES = ["abs_diff", "diff", "sum", "concat"]
UP_CASES = [(1, 1, 1, 1), (2, 3, 9, 7), (1, 64, 1, 3), (3, 2, 5, 257)]          # (h, w) of x, (hs, ws) of the skip
UP_CHANNELS = [(4, 4), (8, 12)]
POOL_CASES = [(64, 64, 64), (65, 63, 64), (2, 3, 64)]                           # (H, W, S)
POOL_S_MAX = 64


def torch_fuse(x1, x2, policy):
    return {"concat": lambda: torch.cat([x1, x2], 1), "sum": lambda: x1 + x2, "diff": lambda: x2 - x1, "abs_diff": lambda: (x1 - x2).abs()}[policy]()


def pair_input(shape, dt, g):
    B = shape[0]
    f = torch.randn(*shape, generator=g).to(dt)
    same = torch.rand(B // 2, *shape[1:], generator=g) < 0.25                    # pixels where x1 == x2 exactly: sign(0) = 0
    f[B // 2:][same] = f[:B // 2][same]
    return f


def to_rows(x):
    """NCHW -> (N*H*W, C)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def from_rows(r, N, H, W):
    return r.reshape(N, H, W, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ refusals
# (entry, the conjunct of its argument check that refuses the call, the source file)
REFUSALS = {"seg_ce_k4097": ("mtp_seg_ce", "K <= 4096", "decode_head.hip"), "pool_fwd_s65": ("mtp_adaptive_avg_pool_fwd", "S <= 64", "decode_head.hip"),
            "pool_bwd_s65": ("mtp_adaptive_avg_pool_bwd", "S <= 64", "decode_head.hip")}
ERR_ARG_TEXT = r"^%s failed: invalid argument$"
