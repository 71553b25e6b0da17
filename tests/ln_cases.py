"""Case tables, inputs and references of the LayerNorm kernels and the row reductions (csrc/layernorm.hip), shared by tests/test_hip_ln_edges.py (GPU)
and tests/test_ln_edges_host.py (CPU).  Plain torch on the CPU: no device; only the refusal table touches the library, through the caller's handle.

* Launch rule: `ln_grid` (forward) and `bwd_cap` (backward) restate the workgroup counts; the row counts of the grid-trip cases are derived from them.
* Exact inputs (`exact_case`): integers and powers of two for which every intermediate of the backward kernels is an f32 number whatever the order of
  summation or the contraction; `exact_bwd` / `exact_res_bwd` return the float64 results together with the terms of every intermediate, which the host
  test proves exact (multiples of 2^-k whose absolute values, times 2^k, sum to less than 2^24).
* One statement of the arithmetic (`ln_math`, `ln_bwd_math`, `res_fwd_math`, `res_bwd_math`), parametrised by dtype: in float64 it is the reference, in
  float32 the RESTATEMENT of the kernel (a sum, a centred second pass, rsqrt, (x - mu) * rs * g + b) from which the regime bounds are derived:

      bound(output) = max(floor, 4 x error of the float32 restatement against float64)          floor = TOL[dtype]; 2e-4 for an f32 dx, dgamma, dbeta, dls

  (the factor test_hip_box_ops.check_iou gives a float32 restatement whose order of summation is not the kernel's).  With `one_pass=True` the variance is
  E[x^2] - mean^2: what the kernels must not do.
* `REGIMES`: the statistics regimes; `regime_case` builds inputs, references, restatement errors and bounds once per (regime, C, dtype).
* `ENTRIES` / `CHECKS` / `REFUSALS`: the argument lists of the entry points, their argument checks restated in source order, and the calls that must be
  refused, each named after the check that refuses it.
"""
import ctypes
import functools

import torch

import sampling_cases as S

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TOL = {F32: 2e-4, BF16: 1.5e-2}          # the project's table (tests/test_hip_edges.py): max error relative to the tensor's max
P_TOL = 2e-4                             # ... and what it holds an f32 dx and the parameter gradients to
EPS = 1e-6
MARGIN = 4.0
INT32_MAX = 2 ** 31 - 1
DTN = {F32: "f32", BF16: "bf16"}


def rel_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape) + 7 * len(shape))
    t = torch.randn(*shape, generator=g) * scale
    return t.to(dtype).float() if dtype == BF16 else t    # values exactly representable in the op's dtype


def rounded(t, dtype):
    return t.to(dtype).float()


# ------------------------------------------------------------------------------------------------ the launch rule
LN_ROWS_PER_WG = 4            # one wave per row, four waves


def ln_grid(rows):
    """layernorm.hip:ln_grid -- workgroups of the forward kernels"""
    return min((rows + 3) // 4, 2048)


BWD_CAPS = [(65536, 512), (262144, 1024), (None, 2048)]      # up to this many rows: at most this many workgroups


def bwd_cap(rows):
    """the cap inside mtp_layernorm_bwd_partial_rows"""
    for upto, cap in BWD_CAPS:
        if upto is None or rows <= upto:
            return cap


def bwd_grid(rows):
    return min((rows + 3) // 4, bwd_cap(rows))


def trips(rows, workgroups):
    """passes of the longest-running wave through `row += gridDim.x * 4`"""
    return -(-rows // (LN_ROWS_PER_WG * workgroups))


_T = LN_ROWS_PER_WG * BWD_CAPS[0][1]                 # rows of one trip of the backward at its smallest cap
BWD_ROWS = [_T, _T + 1, 2 * _T + 1, BWD_CAPS[0][0], BWD_CAPS[0][0] + 1, BWD_CAPS[1][0], BWD_CAPS[1][0] + 1]
_F = LN_ROWS_PER_WG * 2048
FWD_ROWS = [_F, _F + 1, 2 * _F + 1]
C_WIDE = 512
BWD_TRIP_CASES = [(r, 4) for r in BWD_ROWS] + [(r, C_WIDE) for r in BWD_ROWS if r <= 2 * _T + 1]
FWD_TRIP_CASES = [(r, 4) for r in FWD_ROWS] + [(_F + 1, C_WIDE)]
RPS = 7 * 293                 # rows per sample: does not divide 2048, so later trips cross sample boundaries
WIN_GRIDS = [(3, 27, 27), (2, 33, 32)]      # > 2048 tokens: 27 = 3 x 7 + 6 (padding behind only), 33 x 32 (padding in front as well)


# ------------------------------------------------------------------------------------------------ exact inputs
def _pick(gen, values, *shape):
    v = torch.tensor(values, dtype=F32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
def exact_case(rows, C):
    """f32 inputs of the backward kernels (and h / x of the forward ones) for which every intermediate is exact; see the module docstring"""
    assert C & (C - 1) == 0            # the division by C is a shift
    g = torch.Generator().manual_seed(7919 * rows + C)
    ns = -(-rows // RPS)
    c = dict(rows=rows, C=C, ns=ns)
    c["x"] = _ints(g, -2, 2, rows, C)
    c["mean"], c["rstd"] = _pick(g, [-1.0, 0.0, 1.0], rows), _pick(g, [0.5, 1.0, 2.0], rows)
    c["gamma"], c["beta"], c["ls"] = _pick(g, [0.5, 1.0, 2.0, -1.0], C), _pick(g, [-1.0, 0.0, 1.0], C), _pick(g, [0.5, 1.0, 2.0, -1.0], C)
    c["dy"] = _ints(g, -1, 1, rows, C)
    c["dres"], c["extra"] = _ints(g, -3, 3, rows, C), _ints(g, -2, 2, rows, C)
    c["copy_scale"], c["sample_scale"] = _pick(g, [0.0, 0.5, 2.0], ns), _pick(g, [0.0, 0.5, 2.0], ns)
    c["copy_scale"][-1], c["sample_scale"][-1] = 2.0, 0.5           # the last (possibly short) sample counts
    c["pre_g"], c["pre_b"], c["pre_l"] = _ints(g, -5, 5, C), _ints(g, -5, 5, C), _ints(g, -5, 5, C)
    return c


def per_row(scale, rows, rps=RPS):
    return scale.repeat_interleave(rps)[:rows]


def _d(*ts):
    return tuple(None if t is None else t.double() for t in ts)


def exact_bwd(c, wa=None, fused=False, accumulate=False):
    """float64 results of ln_bwd_kernel on an exact case and the terms of every intermediate: [(name, [tensors summed together], axis of a further sum or
    None)].  wa: the window addend already gathered per row; fused: with dres, extra and the scaled copy; accumulate: onto pre_g / pre_b"""
    C = c["C"]
    dy, x, mean, rstd, gamma = _d(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"])
    m, r = mean[:, None].expand_as(x), rstd[:, None]
    xh = (x - m) * r
    dvt = [dy] + ([wa.double()] if wa is not None else [])
    dv = sum(dvt)
    d = dv * gamma
    c1, c2 = (d * xh).sum(1, keepdim=True) / C, d.sum(1, keepdim=True) / C
    core = [d * r, -(xh * c1) * r, (-c2 * r).expand_as(x)]
    add = list(_d(c["dres"], c["extra"])) if fused else []
    dx = sum(core + add)
    pre = _d(c["pre_g"], c["pre_b"]) if accumulate else (torch.zeros(C, dtype=F64),) * 2
    res = dict(dx=dx, dgamma=(dv * xh).sum(0) + pre[0], dbeta=dv.sum(0) + pre[1])
    terms = [("x - mean", [x, m], None), ("xhat", [xh], None), ("dy + win_add", dvt, None), ("dgamma", [dv * xh, pre[0][None]], 0),
             ("dbeta", [dv, pre[1][None]], 0), ("d", [d], None), ("s1", [d * xh], 1), ("s2", [d], 1), ("c1", [c1], None), ("c2", [c2], None),
             ("xhat c1", [xh * c1], None), ("d - xhat c1 - c2", [d, xh * c1, c2.expand_as(x)], None), ("dx", core + add, None)]
    if fused:
        res["dx_copy"] = dx * per_row(c["copy_scale"].double(), c["rows"])[:, None]
        terms.append(("dx_copy", [res["dx_copy"]], None))
    return res, terms


def exact_res_bwd(c):
    """the same for ln_res_bwd_kernel with sample_scale; the three parameter gradients accumulate onto pre_g / pre_b / pre_l"""
    C = c["C"]
    dout, h, mean, rstd, gamma, beta, ls = _d(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], c["beta"], c["ls"])
    sc = per_row(c["sample_scale"].double(), c["rows"])[:, None]
    m, r = mean[:, None].expand_as(h), rstd[:, None]
    xh = (h - m) * r
    sd = sc * dout
    z = [xh * gamma, beta.expand_as(h)]
    dy = sd * ls
    d = dy * gamma
    c1, c2 = (d * xh).sum(1, keepdim=True) / C, d.sum(1, keepdim=True) / C
    core = [d * r, -(xh * c1) * r, (-c2 * r).expand_as(h)]
    pg, pb, pl = _d(c["pre_g"], c["pre_b"], c["pre_l"])
    res = dict(dh=sum(core), dgamma=(dy * xh).sum(0) + pg, dbeta=dy.sum(0) + pb, dls=(sd * sum(z)).sum(0) + pl)
    terms = [("h - mean", [h, m], None), ("xhat", [xh], None), ("s dout", [sd], None), ("z", z, None), ("dls", [sd * z[0], sd * z[1], pl[None]], 0),
             ("dy", [dy], None), ("dgamma", [dy * xh, pg[None]], 0), ("dbeta", [dy, pb[None]], 0), ("d", [d], None), ("s1", [d * xh], 1), ("s2", [d], 1),
             ("c1", [c1], None), ("c2", [c2], None), ("xhat c1", [xh * c1], None), ("d - xhat c1 - c2", [d, xh * c1, c2.expand_as(h)], None), ("dh", core, None)]
    return res, terms


def dyadic_k(t, kmax=40):
    """the smallest k with t * 2^k all integers (t float64); None if there is none up to kmax"""
    for k in range(kmax + 1):
        s = t * 2.0 ** k
        if torch.equal(s, s.round()):
            return k
    return None


def exactness(terms):
    """(k, worst sum of |terms| * 2^k) of one intermediate: exact in f32 in any order and under any contraction if k is not None and the sum < 2^24"""
    ts, axis = terms[1], terms[2]
    ks = [dyadic_k(t) for t in ts]
    if any(k is None for k in ks):
        return None, float("inf")
    k = max(ks)
    tot = None
    for t in ts:
        a = t.abs() * 2.0 ** k
        if axis is not None:
            a = a.sum(axis, keepdim=True)
        tot = a if tot is None else tot + a
    return k, float(tot.max())


def window_rows(B, Hp, Wp):
    """window index of every token row of a (B, Hp, Wp) grid, and the window count"""
    _, _, nh, nw = S.windows(Hp, Wp)
    return S.token_windows(B, Hp, Wp), B * nh * nw


@functools.lru_cache(maxsize=None)
def exact_win_case(B, Hp, Wp, C):
    c = dict(exact_case(B * Hp * Wp, C))
    win, nwin = window_rows(B, Hp, Wp)
    g = torch.Generator().manual_seed(B * 1000 + Hp * Wp + C)
    c["win_add"], c["win"] = _ints(g, -1, 1, nwin, C), win
    return c


@functools.lru_cache(maxsize=None)
def exact_fwd_case(rows, C):
    """x = integers in [-2, 2] plus a row-dependent integer offset: the mean (a sum of integers over a power of two) is exact and differs from row to row, so
    a row read or written at another index cannot pass"""
    assert C & (C - 1) == 0
    g = torch.Generator().manual_seed(104729 * rows + C)
    off = (torch.arange(rows) % 251 - 125).float()
    assert (LN_ROWS_PER_WG * 2048) % 251 and (LN_ROWS_PER_WG * 512) % 251         # a row one trip away has another offset
    c = dict(rows=rows, C=C, x=_ints(g, -2, 2, rows, C) + off[:, None])
    c["gamma"], c["beta"], c["ls"] = 1 + 0.1 * rnd(C, seed=1), 0.1 * rnd(C, seed=2), 0.5 * rnd(C, seed=3)
    c["res"] = torch.randn(rows, C, generator=g)
    c["sample_scale"] = _pick(g, [0.0, 1.25, 0.5], -(-rows // RPS))
    y, mu, rs, _ = ln_math(c["x"], c["gamma"], c["beta"], F64)
    c["ref"] = dict(y=y, mean=mu, rstd=rs, out=c["res"].double() + per_row(c["sample_scale"].double(), rows)[:, None] * c["ls"].double() * y)
    return c


# ------------------------------------------------------------------------------------------------ the arithmetic, once
def gelu_math(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.70710678118654752440))


def dgelu_math(z):
    return 0.5 * (1.0 + torch.erf(z * 0.70710678118654752440)) + z * 0.39894228040143267794 * torch.exp(-0.5 * z * z)


def ln_math(x, g, b, dtype, one_pass=False, gelu=False):
    """(y, mean, rstd, z) in `dtype`: float64 = the reference, float32 = the restatement of ln_fwd_kernel.  one_pass: var = E[x^2] - mean^2, clamped at 0"""
    x, g, b = x.to(dtype), g.to(dtype), b.to(dtype)
    C = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / C
    if one_pass:
        var = ((x * x).sum(-1, keepdim=True) / C - mu * mu).clamp_min(0)
    else:
        var = ((x - mu) ** 2).sum(-1, keepdim=True) / C
    rs = torch.rsqrt(var + EPS)
    z = (x - mu) * rs * g + b
    return (gelu_math(z) if gelu else z), mu.squeeze(-1), rs.squeeze(-1), z


def ln_bwd_math(dy, x, mu, rs, g, dtype, b=None, gelu=False):
    """(dx, dgamma, dbeta) of ln_bwd_kernel without its addends"""
    dy, x, mu, rs, g = (t.to(dtype) for t in (dy, x, mu, rs, g))
    C = x.shape[-1]
    xh = (x - mu[:, None]) * rs[:, None]
    dv = dy * dgelu_math(xh * g + b.to(dtype)) if gelu else dy
    d = dv * g
    c1, c2 = (d * xh).sum(-1, keepdim=True) / C, d.sum(-1, keepdim=True) / C
    return (d - xh * c1 - c2) * rs[:, None], (dv * xh).sum(0), dv.sum(0)


def res_fwd_math(h, g, b, x, ls, srow, dtype, one_pass=False):
    """(out, mean, rstd) of ln_res_fwd_kernel; srow: the sample scale of every row"""
    y, mu, rs, _ = ln_math(h, g, b, dtype, one_pass=one_pass)
    return x.to(dtype) + srow.to(dtype)[:, None] * ls.to(dtype) * y, mu, rs


def res_bwd_math(dout, h, mu, rs, g, b, ls, srow, dtype):
    """(dh, dgamma, dbeta, dls) of ln_res_bwd_kernel"""
    dout, h, mu, rs, g, b, ls, srow = (t.to(dtype) for t in (dout, h, mu, rs, g, b, ls, srow))
    C = h.shape[-1]
    xh = (h - mu[:, None]) * rs[:, None]
    sd = srow[:, None] * dout
    dls = (sd * (xh * g + b)).sum(0)
    dy = sd * ls
    d = dy * g
    c1, c2 = (d * xh).sum(-1, keepdim=True) / C, d.sum(-1, keepdim=True) / C
    return (d - xh * c1 - c2) * rs[:, None], (dy * xh).sum(0), dy.sum(0), dls


# ------------------------------------------------------------------------------------------------ width seams
WIDTHS = [252, 256, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1540, 2044, 2048]
SEAM_ROWS = [5, 9]            # the last workgroup has one live wave: three waves contribute zeros through the LDS reduction
GELU_WIDTHS = [252, 516, 1028, 2048]
FWD_COMBOS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)]                              # (x, y)
BWD_COMBOS = [(BF16, F32, F32), (F32, F32, F32), (BF16, BF16, BF16), (F32, BF16, BF16)]        # (dy, x, dx); the last: InternImage's dw-conv branch
LN_MVS = [1, 2, 3, 4, 6, 8]


def mv_of(C):
    """MTP_LN_MV: the float4 groups per lane of the instantiation a row of C channels runs on"""
    mv = (C // 4 + 63) // 64
    return mv if mv <= 4 else 6 if mv <= 6 else 8


def masked_lanes(C):
    """lanes x groups of the instantiation that lie past the row's end (clamped loads, masked stores)"""
    return 64 * mv_of(C) - C // 4


# ------------------------------------------------------------------------------------------------ regimes
REGIME_ROWS = 33
REGIME_WIDTHS = [4, 260, 1024, 2048]
CONSTANTS = [3.0, -0.5, 1024.0]


def _regime(name, n):
    rows, C = n.shape
    if name == "offset_1e3":
        return 1000.0 + n
    if name == "offset_neg_small_std":
        return -300.0 + 0.05 * n
    if name == "spike":
        x = n.clone()
        x[torch.arange(rows), (5 * torch.arange(rows) + 1) % C] = 3000.0
        return x
    if name == "near_eps":
        return 1.0 + 1e-3 * n
    if name == "tiny":
        return 1e-4 * n
    if name == "big":
        return 1e4 * n
    if name == "constant":
        return torch.tensor(CONSTANTS)[torch.arange(rows) % 3][:, None].expand(rows, C).contiguous()
    if name == "normal":
        return n.clone()
    raise KeyError(name)


REGIMES = ["offset_1e3", "offset_neg_small_std", "spike", "near_eps", "tiny", "big", "constant"]
ONE_PASS_MUST_MISS = ["offset_1e3", "offset_neg_small_std", "near_eps"]
ONE_PASS_FACTOR = 10.0


def mean_err(mean, mean_ref, rstd_ref):
    """the error of a mean in units of the row's standard deviation: what it does to xhat"""
    return float(((mean.double() - mean_ref.double()).abs() * rstd_ref.double()).max())


def _bound(floor, restated):
    return max(floor, MARGIN * restated)


def _errs(got, ref):
    """output -> error of `got` against `ref` (dicts); 'mean' in units of the standard deviation, everything else relative to the reference's max"""
    return {k: (mean_err(got[k], ref[k], ref["rstd"]) if k == "mean" else rel_err(got[k], ref[k])) for k in got}


def floors(act):
    """output -> the project's tolerance: TOL of the output's dtype; 2e-4 for an f32 dx and the parameter gradients"""
    f = dict(y=TOL[act], y_gelu=TOL[act], mean=TOL[F32], rstd=TOL[F32], dx=(P_TOL if act == F32 else TOL[BF16]), dgamma=P_TOL, dbeta=P_TOL,
             dx_gelu=(P_TOL if act == F32 else TOL[BF16]), dgamma_gelu=P_TOL, dbeta_gelu=P_TOL,
             out=TOL[F32], out_act=TOL[act], res_mean=TOL[F32], res_rstd=TOL[F32], dh=TOL[act], res_dgamma=P_TOL, res_dbeta=P_TOL, dls=P_TOL)
    return f


def evaluate(inp, dtype, act, one_pass=False):
    """every output of the five kernels on the inputs `inp`, computed in `dtype` (float64: reference; float32: restatement, its activation outputs rounded
    to `act` as the kernel rounds them).  The backward runs on the statistics of the same evaluation, as the GPU test runs it on the kernel's own."""
    cast = (lambda t: rounded(t, act).double()) if (dtype == F32 and act == BF16) else (lambda t: t.double())
    x, g, b, dy = inp["x"], inp["gamma"], inp["beta"], inp["dy"]
    y, mu, rs, _ = ln_math(x, g, b, dtype, one_pass=one_pass)
    yg = ln_math(x, g, b, dtype, one_pass=one_pass, gelu=True)[0]
    dx, dg, db = ln_bwd_math(dy, x, mu, rs, g, dtype)
    dxg, dgg, dbg = ln_bwd_math(dy, x, mu, rs, g, dtype, b=b, gelu=True)
    out, rmu, rrs = res_fwd_math(x, g, b, inp["res"], inp["ls"], inp["srow"], dtype, one_pass=one_pass)
    dh, rdg, rdb, dls = res_bwd_math(inp["dout"], x, rmu, rrs, g, b, inp["ls"], inp["srow"], dtype)
    r = dict(y=cast(y), y_gelu=cast(yg), mean=mu.double(), rstd=rs.double(), dx=cast(dx), dgamma=dg.double(), dbeta=db.double(),
             dx_gelu=cast(dxg), dgamma_gelu=dgg.double(), dbeta_gelu=dbg.double(),
             out=out.double(), out_act=cast(out), res_mean=rmu.double(), res_rstd=rrs.double(), dh=cast(dh), res_dgamma=rdg.double(), res_dbeta=rdb.double(),
             dls=dls.double())
    return r


def _case_from(x, C, act, seed, gelu_spread=False):
    rows = x.shape[0]
    inp = dict(x=rounded(x, act), dy=rnd(rows, C, dtype=act, seed=seed + 1), dout=rnd(rows, C, seed=seed + 2), res=rnd(rows, C, seed=seed + 3),
               gamma=1 + 0.1 * rnd(C, seed=seed + 4), beta=0.1 * rnd(C, seed=seed + 5), ls=0.5 * rnd(C, seed=seed + 6))
    if gelu_spread:       # z = xhat * gamma + beta over [-12, 12]: gamma near +-4; channel 0 has gamma = beta = 0, i.e. z = 0 exactly
        inp["gamma"] = torch.tensor([3.5, 4.0, 4.5, -4.0])[torch.arange(C) % 4] + 0.01 * rnd(C, seed=seed + 4)
        inp["gamma"][0], inp["beta"][0] = 0.0, 0.0
    ss = (torch.arange((rows + 1) // 2) % 3 != 1).float() / 0.8
    inp["sample_scale"], inp["rps"], inp["srow"] = ss, 2, per_row(ss, rows, 2)
    ref, rst = evaluate(inp, F64, act), evaluate(inp, F32, act)
    # the reference's mean / rstd keys of the residual kernel are measured like the plain ones
    err = _errs(rst, dict(ref, rstd=ref["rstd"]))
    err["res_mean"] = mean_err(rst["res_mean"], ref["res_mean"], ref["res_rstd"])
    fl = floors(act)
    return dict(inp=inp, ref=ref, restated=err, bound={k: _bound(fl[k], err[k]) for k in err}, act=act, C=C)


@functools.lru_cache(maxsize=None)
def regime_case(name, C, act):
    n = torch.randn(REGIME_ROWS, C, generator=torch.Generator().manual_seed(REGIMES.index(name) * 10007 + C))
    return _case_from(_regime(name, n), C, act, seed=100 * REGIMES.index(name) + C)


@functools.lru_cache(maxsize=None)
def gelu_case(C, act):
    n = torch.randn(REGIME_ROWS, C, generator=torch.Generator().manual_seed(31337 + C))
    return _case_from(n, C, act, seed=9000 + C, gelu_spread=True)


def kernel_errors(case, got):
    """output -> error of the kernel's outputs `got` (a dict with some of the keys of the reference, CPU tensors) against the case's float64 reference"""
    ref = case["ref"]
    out = {}
    for k, v in got.items():
        out[k] = mean_err(v, ref[k], ref["rstd" if k == "mean" else "res_rstd"]) if k in ("mean", "res_mean") else rel_err(v.float(), ref[k])
    return out


# ------------------------------------------------------------------------------------------------ row reductions
RED_ROWS = [1, 7, 8, 9, 12, 13, 14, 15, 16, 17, 31, 33, 512, 513, 2049]     # column_sum's remainders after 8 and 4 (14: the one with two single rows); rows / 16 of the batched split; a workload's partial rows
RED_COLS = [1, 255, 256, 257, 4100]                                     # 4100: 17 column blocks, split counts that are no power of two
RED_PAD = 8                                                             # the column slice: ld = cols + 8
REDUCE_BATCH_MAX = 32
RED_BATCHES = [(n, rows, cols) for n in (1, 2, 32, 33) for rows, cols in ((15, 257), (16, 1), (17, 257), (33, 4100), (513, 255))]


def plain_splits(rows, cols):
    """mtp_reduce_rows_f32: (row pieces, rows per piece)"""
    cb = (cols + 255) // 256
    s = max(1, min(1024 // cb, rows))
    rpb = -(-rows // s)
    return -(-rows // rpb), rpb


def batched_splits(rows, cols, n):
    """mtp_reduce_rows_batched_f32: (row pieces, rows per piece)"""
    cb = (cols + 255) // 256
    s = max(1, min(2048 // (cb * n), rows // 16))
    rpb = -(-rows // s)
    return -(-rows // rpb), rpb


def column_sum_passes(nrows):
    """column_sum over nrows rows: (passes of 8, passes of 4, single rows)"""
    return nrows // 8, nrows % 8 // 4, nrows % 4


# ------------------------------------------------------------------------------------------------ refusals
# argument lists in ABI order.  kind: in / out = pointer the kernel would read / write; i = integer; f = float; s = stream; ins / outs = pointer arrays
def _spec(s):
    return [tuple(a.split(":")) for a in s.split()]


ENTRIES = {
    "mtp_layernorm_fwd": _spec("x:in x_dtype:i gamma:in beta:in y:out y_dtype:i mean:out rstd:out rows:i C:i eps:f fuse_gelu:i stream:s"),
    "mtp_layernorm_bwd": _spec("dy:in dy_dtype:i x:in x_dtype:i mean:in rstd:in gamma:in beta:in fuse_gelu:i dres:in extra:in dx:out dx_dtype:i dx_copy:out "
                               "copy_dtype:i copy_scale:in rows_per_sample:i dgamma_part:out dbeta_part:out part_ld:i rows:i C:i stream:s"),
    "mtp_layernorm_bwd_win": _spec("dy:in dy_dtype:i x:in x_dtype:i mean:in rstd:in gamma:in dres:in extra:in dx:out dx_dtype:i dx_copy:out copy_dtype:i "
                                   "copy_scale:in rows_per_sample:i dgamma_part:out dbeta_part:out part_ld:i rows:i C:i win_add:in B:i Hp:i Wp:i stream:s"),
    "mtp_layernorm_residual_fwd": _spec("h:in dtype:i gamma:in beta:in x:in layer_scale:in sample_scale:in rows_per_sample:i out:out out_act:out mean:out "
                                        "rstd:out rows:i C:i eps:f stream:s"),
    "mtp_layernorm_residual_bwd": _spec("dout:in h:in dtype:i mean:in rstd:in gamma:in beta:in layer_scale:in sample_scale:in rows_per_sample:i dh:out part:out "
                                        "rows:i C:i stream:s"),
    "mtp_reduce_rows_f32": _spec("part:in ld:i out:out rows:i C:i accumulate:i stream:s"),
    "mtp_reduce_rows_batched_f32": _spec("parts:ins outs:outs n:i ld:i rows:i C:i accumulate:i stream:s"),
    "mtp_reduce_rows_t_batched_f32": _spec("parts:ins outs:outs n:i ld:i rows:i R:i C:i accumulate:i stream:s"),
}
# a call every check lets through: rows = B Hp Wp = 8 tokens of 8 channels, all f32; the optional pointers are NULL
VALID = dict(rows=8, C=8, R=1, eps=EPS, fuse_gelu=0, x_dtype=0, y_dtype=0, dy_dtype=0, dx_dtype=0, copy_dtype=0, dtype=0, rows_per_sample=0, part_ld=0,
             B=1, Hp=2, Wp=4, ld=8, n=2, accumulate=0, null_at=None)
OPTIONAL = {"dres", "extra", "dx_copy", "copy_scale", "sample_scale"}
SUPPORTED_BWD = {(1, 0, 0), (0, 0, 0), (1, 1, 1), (0, 1, 1)}          # (dy, x, dx) dtypes; the window form has the first two only
ARG, UNSUPPORTED = -1, -2
ERR_TEXT = {ARG: r"^%s failed: invalid argument$", UNSUPPORTED: r"^%s failed: unsupported configuration$"}


def resolve(entry, over):
    """name -> value of every argument of a call: integers as given, pointers as True (present) / False (NULL)"""
    a = dict(VALID)
    for name, kind in ENTRIES[entry]:
        if kind in ("in", "out", "ins", "outs"):
            a[name] = name not in OPTIONAL
    a.update(over)
    return a


def _ld_eff(a):
    return a["part_ld"] if a["part_ld"] != 0 else a["C"]


def _need(*names):
    return lambda a: not all(a[n] for n in names)


_SIZE = [("rows <= 0", lambda a: a["rows"] <= 0), ("rows > INT32_MAX", lambda a: a["rows"] > INT32_MAX), ("C <= 0", lambda a: a["C"] <= 0),
         ("(C % 4)", lambda a: a["C"] % 4 != 0), ("C > 256 * MAXV", lambda a: a["C"] > 2048)]
_PART = [("part_ld < C", lambda a: _ld_eff(a) < a["C"]), ("(part_ld % 4)", lambda a: _ld_eff(a) % 4 != 0)]
_COPY = [("dx_copy && copy_dtype != dy_dtype", lambda a: a["dx_copy"] and a["copy_dtype"] != a["dy_dtype"])]
_SS = [("sample_scale && rows_per_sample <= 0", lambda a: a["sample_scale"] and a["rows_per_sample"] <= 0)]
_BATCH = [("!parts", _need("parts")), ("!outs", _need("outs")), ("n <= 0", lambda a: a["n"] <= 0), ("n > MTP_REDUCE_BATCH_MAX", lambda a: a["n"] > REDUCE_BATCH_MAX),
          ("rows <= 0", lambda a: a["rows"] <= 0)]
_NULL_ENTRY = [("!parts[i] || !outs[i]", lambda a: a["null_at"] is not None)]
_BWD_PTRS = ("dy", "x", "mean", "rstd", "gamma", "dx", "dgamma_part", "dbeta_part")
# entry -> its checks in source order: (the text of the check in the source, the line of layernorm.hip that holds it, what it returns, the check restated)
CHECKS = {
    "mtp_layernorm_fwd": [(t, 491, ARG, p) for t, p in [("!x || !gamma || !beta || !y", _need("x", "gamma", "beta", "y"))] + _SIZE[:1] + _SIZE[2:]]
    + [("return MTP_ERR_UNSUPPORTED;", 497, UNSUPPORTED, lambda a: a["x_dtype"] not in (0, 1) or a["y_dtype"] not in (0, 1))],
    "mtp_layernorm_bwd": [(t, 553, ARG, p) for t, p in _PART]
    + [(t, 554, ARG, p) for t, p in [("!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma_part || !dbeta_part", _need(*_BWD_PTRS))] + _SIZE]
    + [("fuse_gelu && !beta", 555, ARG, lambda a: a["fuse_gelu"] and not a["beta"])] + [(t, 556, ARG, p) for t, p in _COPY]
    + [("return MTP_ERR_UNSUPPORTED;", 566, UNSUPPORTED, lambda a: (a["dy_dtype"], a["x_dtype"], a["dx_dtype"]) not in SUPPORTED_BWD)],
    "mtp_layernorm_bwd_win": [(t, 575, ARG, p) for t, p in _PART]
    + [(t, 576, ARG, p) for t, p in [("!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma_part || !dbeta_part", _need(*_BWD_PTRS))] + _SIZE]
    + [(t, 577, ARG, p) for t, p in [("!win_add", _need("win_add")), ("B <= 0 || Hp <= 0 || Wp <= 0", lambda a: min(a["B"], a["Hp"], a["Wp"]) <= 0),
                                      ("B * Hp * Wp != rows", lambda a: a["B"] * a["Hp"] * a["Wp"] != a["rows"])]]
    + [(t, 578, ARG, p) for t, p in _COPY]
    + [("return MTP_ERR_UNSUPPORTED;", 586, UNSUPPORTED, lambda a: (a["dy_dtype"], a["x_dtype"], a["dx_dtype"]) not in {(1, 0, 0), (0, 0, 0)})],
    "mtp_layernorm_residual_fwd": [(t, 520, ARG, p) for t, p in [("!h || !gamma || !beta || !x || !layer_scale || !out || !mean || !rstd",
                                                                  _need("h", "gamma", "beta", "x", "layer_scale", "out", "mean", "rstd"))] + _SIZE]
    + [(t, 521, ARG, p) for t, p in _SS] + [("return for_act(dtype,", 523, UNSUPPORTED, lambda a: a["dtype"] not in (0, 1))],
    "mtp_layernorm_residual_bwd": [(t, 531, ARG, p) for t, p in [("!dout || !h || !mean || !rstd || !gamma || !beta || !layer_scale || !dh || !part",
                                                                  _need("dout", "h", "mean", "rstd", "gamma", "beta", "layer_scale", "dh", "part"))] + _SIZE]
    + [(t, 532, ARG, p) for t, p in _SS] + [("return for_act(dtype,", 534, UNSUPPORTED, lambda a: a["dtype"] not in (0, 1))],
    "mtp_reduce_rows_f32": [(t, 590, ARG, p) for t, p in [("!part || !out", _need("part", "out")), ("rows <= 0", lambda a: a["rows"] <= 0),
                                                           ("C <= 0", lambda a: a["C"] <= 0), ("ld < C", lambda a: a["ld"] < a["C"])]],
    "mtp_reduce_rows_batched_f32": [(t, 608, ARG, p) for t, p in _BATCH + [("C <= 0", lambda a: a["C"] <= 0), ("ld < C", lambda a: a["ld"] < a["C"])]]
    + [(t, 612, ARG, p) for t, p in _NULL_ENTRY],
    "mtp_reduce_rows_t_batched_f32": [(t, 636, ARG, p) for t, p in _BATCH + [("R <= 0", lambda a: a["R"] <= 0), ("C <= 0", lambda a: a["C"] <= 0),
                                                                            ("ld < R * C", lambda a: a["ld"] < a["R"] * a["C"])]]
    + [(t, 640, ARG, p) for t, p in _NULL_ENTRY],
}


def first_check(entry, over):
    """(text, line, return value) of the first check of `entry` that refuses the call, or None"""
    a = resolve(entry, over)
    for text, line, rc, pred in CHECKS[entry]:
        if pred(a):
            return text, line, rc
    return None


def _refusals():
    """(entry, what differs from VALID, the check that must refuse it)"""
    out = []
    ln = ["mtp_layernorm_fwd", "mtp_layernorm_bwd", "mtp_layernorm_bwd_win", "mtp_layernorm_residual_fwd", "mtp_layernorm_residual_bwd"]
    for en in ln:
        bwd = en in ("mtp_layernorm_bwd", "mtp_layernorm_bwd_win")
        out += [(en, dict(C=0), "C <= 0"), (en, dict(C=-4), "C <= 0"), (en, dict(C=2052), "C > 256 * MAXV"),
                (en, dict(C=6, part_ld=8) if bwd else dict(C=6), "(C % 4)"), (en, dict(rows=0, B=0), "rows <= 0")]
        if en != "mtp_layernorm_fwd":
            out.append((en, dict(rows=INT32_MAX + 1, B=INT32_MAX + 1, Hp=1, Wp=1), "rows > INT32_MAX"))
        if bwd:
            out += [(en, dict(part_ld=4), "part_ld < C"), (en, dict(part_ld=10), "(part_ld % 4)"), (en, dict(C=6), "(part_ld % 4)"),      # part_ld 0 means C
                    (en, dict(dx_copy=True, copy_dtype=1), "dx_copy && copy_dtype != dy_dtype"),
                    (en, dict(dy_dtype=1, dx_copy=True, copy_dtype=0), "dx_copy && copy_dtype != dy_dtype"),
                    (en, dict(dy_dtype=1, x_dtype=1, dx_dtype=0), "return MTP_ERR_UNSUPPORTED;"),            # bf16 dy and x with an f32 dx
                    (en, dict(dy_dtype=0, x_dtype=0, dx_dtype=1), "return MTP_ERR_UNSUPPORTED;"),
                    (en, dict(dy_dtype=7), "return MTP_ERR_UNSUPPORTED;"), (en, dict(dx=False), "!dy || !x || !mean || !rstd || !gamma || !dx || !dgamma_part || !dbeta_part")]
    out += [("mtp_layernorm_bwd", dict(fuse_gelu=1, beta=False), "fuse_gelu && !beta"),
            ("mtp_layernorm_bwd_win", dict(dy_dtype=1, x_dtype=1, dx_dtype=1), "return MTP_ERR_UNSUPPORTED;"),   # the plain form has this combination, the window form not
            ("mtp_layernorm_bwd_win", dict(B=2), "B * Hp * Wp != rows"), ("mtp_layernorm_bwd_win", dict(rows=12), "B * Hp * Wp != rows"),
            ("mtp_layernorm_bwd_win", dict(Hp=0), "B <= 0 || Hp <= 0 || Wp <= 0"), ("mtp_layernorm_bwd_win", dict(B=-1, Hp=-2), "B <= 0 || Hp <= 0 || Wp <= 0"),
            ("mtp_layernorm_bwd_win", dict(win_add=False), "!win_add"),
            ("mtp_layernorm_fwd", dict(x_dtype=2), "return MTP_ERR_UNSUPPORTED;"), ("mtp_layernorm_fwd", dict(y_dtype=7), "return MTP_ERR_UNSUPPORTED;"),
            ("mtp_layernorm_fwd", dict(y=False), "!x || !gamma || !beta || !y")]
    for en in ("mtp_layernorm_residual_fwd", "mtp_layernorm_residual_bwd"):
        out += [(en, dict(sample_scale=True, rows_per_sample=0), "sample_scale && rows_per_sample <= 0"),
                (en, dict(sample_scale=True, rows_per_sample=-2), "sample_scale && rows_per_sample <= 0"), (en, dict(dtype=2), "return for_act(dtype,")]
    out += [("mtp_reduce_rows_f32", dict(ld=4), "ld < C"), ("mtp_reduce_rows_f32", dict(rows=0), "rows <= 0"), ("mtp_reduce_rows_f32", dict(rows=-3), "rows <= 0"),
            ("mtp_reduce_rows_f32", dict(C=0, ld=0), "C <= 0"), ("mtp_reduce_rows_f32", dict(out=False), "!part || !out")]
    for en in ("mtp_reduce_rows_batched_f32", "mtp_reduce_rows_t_batched_f32"):
        out += [(en, dict(ld=4), "ld < C" if "_t_" not in en else "ld < R * C"), (en, dict(rows=0), "rows <= 0"), (en, dict(n=0), "n <= 0"),
                (en, dict(n=REDUCE_BATCH_MAX + 1), "n > MTP_REDUCE_BATCH_MAX"), (en, dict(null_at=1), "!parts[i] || !outs[i]"),
                (en, dict(n=REDUCE_BATCH_MAX, null_at=REDUCE_BATCH_MAX - 1), "!parts[i] || !outs[i]"), (en, dict(C=-4, ld=-4), "C <= 0")]
    return out


REFUSALS = _refusals()


def refusal_id(r):
    return "%s-%s" % (r[0].replace("mtp_", ""), "-".join("%s=%s" % kv for kv in sorted(r[1].items())))


def refused_call(lib, entry, over, ptr, stream=None):
    """the return value of `entry` called with VALID changed by `over`.  ptr(name, kind, i) gives the address of a present pointer argument (i: its index in a
    pointer array, else None); a call that is refused reads none of them"""
    a = resolve(entry, over)
    args, keep = [], []
    for name, kind in ENTRIES[entry]:
        v = a.get(name)
        if kind in ("in", "out"):
            args.append(ptr(name, kind, None) if v else None)
        elif kind in ("ins", "outs"):
            if not v:
                args.append(None)
                continue
            n = max(1, a["n"])
            arr = (ctypes.c_void_p * n)(*[None if (a["null_at"] == i and kind == "outs") else ptr(name, kind[:-1], i) for i in range(n)])
            keep.append(arr)
            args.append(arr)
        elif kind == "s":
            args.append(stream)
        else:
            args.append(v)
    return getattr(lib, entry)(*args)


# ------------------------------------------------------------------------------------------------ restated source lines
RESTATES = [      # (what restates it, line of mtp_amd/csrc/layernorm.hip, what that line holds)
    ("ln_grid", 439, "int64_t nb = (rows + 3) / 4;"), ("ln_grid", 440, "return (int)(nb < 2048 ? nb : 2048);"),
    ("trips", 34, "row += (int64_t)gridDim.x * 4"), ("trips", 93, "row += (int64_t)gridDim.x * 4"), ("trips", 205, "row += (int64_t)gridDim.x * 4"),
    ("trips", 268, "row += (int64_t)gridDim.x * 4"),
    ("bwd_cap", 544, "const int64_t cap = rows > 262144 ? 2048 : rows > 65536 ? 1024 : 512;"),
    ("mv_of", 448, "const int mv_ = (int)(((C_) / 4 + 63) / 64);"), ("mv_of", 452, "else if (mv_ == 4) { CALL(4); }"), ("mv_of", 453, "else if (mv_ <= 6) { CALL(6); }"),
    ("mv_of", 454, "else { CALL(8); }"),
    ("column_sum_passes", 334, "for (; r + 8 <= r1; r += 8) {"), ("column_sum_passes", 340, "for (; r + 4 <= r1; r += 4) {"),
    ("plain_splits", 597, "int64_t splits = 1024 / col_blocks;"), ("plain_splits", 599, "if (splits > rows) splits = rows;"),
    ("batched_splits", 625, "int64_t splits = 2048 / (col_blocks * n);"), ("batched_splits", 626, "if (splits > rows / 16) splits = rows / 16;"),
]
