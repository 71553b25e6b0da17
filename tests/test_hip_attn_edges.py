"""GPU: the attention kernels at the smallest grid each kernel family takes, in softmax regimes the other tests never enter, every buffer out of the
guard arena (tests/guard.py) as in test_hip_edges.py.  References: the oracles of oracle/vit_rvsa_oracle.py in float64 on the CPU, from the
dtype-rounded inputs, gradients by autograd.  Every case asserts the kernel family that runs (ops.full_attn_kernel / ops.rvsa_attn_kernel).

Regimes (inputs stay exactly representable in the op's dtype: they are rounded once more after the construction):
  R0  the recipe of test_hip_ops.py (control)                 R1  q, k x 4 and planted maxima: one query direction d is copied into a few query rows and
  R2  q = 3|q|, k = -3|k|: every logit far below zero             2 d into the LAST key of image 0 / the FIRST key of the last image (full attention; the
  R3  q = 3|q|, k = 3|k|: every logit far above zero              RVSA kernels hold all 49 keys of a window in one block: there R1 is the x 4 alone)
  R4  qkv / 4, tables x 8: the bias terms dominate            R4z qkv / 4, tables exactly zero
  R5  (RVSA) sampling offsets of 50: every sample outside the map; o, dk, dv and dsamp are exactly zero        R5m (RVSA) samp = 3 randn
With B = 3 the last image's v and dout carry a factor 1 / 64 (exact), so its slices are 64 resp. 4096 times smaller than the others.

Errors are maxima normalised PER (image, head) SLICE for o, lse and the dq / dk / dv parts of dqkv (a whole-tensor norm would hide the small image);
table gradients and dsamp are normalised over the whole tensor.  Two normalisers have a floor, both by reasoning, neither from a kernel's output:
  * lse is a logarithm: its rounding error is absolute (that of the logits), so a slice whose |lse| stays below 1 is measured against 1;
  * on a grid of one or two tokens dq and dk cancel: with one key they are exactly zero (softmax = 1, dP = delta), with two dS = p0 p1 dout.(v0 - v1)
    is what is left of p0 (dP0 - delta) once the softmax saturates.  What a kernel returns there is the rounding of the TERMS dP and delta, so the
    slice is measured against at least their scale  max sum |dout| |v| * max(|q|, |k|) * scale  (the argument of bn_dx_small_rows_bound);
  * a relative-position table of ONE row (Hp = 1 resp. Wp = 1) adds the same term to every key of a row: its gradient is exactly zero, a kernel's is
    the rounding of the sums that make up the other table's gradient, against whose size it is then measured;
  * a slice whose reference is exactly zero (RVSA windows whose samples all fall outside the map) must be exactly zero.
Bounds: the project's table (outputs 2e-4 / 1.5e-2, table gradients and dsamp ten times that, lse 1e-4 / 5e-3) unless EXCEPTIONS below names the
(kind, regime, output): then 4 x the error measured on the CPU by tests/test_attn_edges_host.py (float32 oracle vs float64 oracle for f32; for bf16 an
emulation that rounds P, dS and the outputs to bf16 -- for RVSA also the gathered K / V rows and the tables, bf16 MFMA operands that are no inputs),
which that file re-measures and asserts."""
import functools

import pytest
import torch

import guard
from conftest import rel_err, record_parity
from oracle import vit_rvsa_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
HD = 64
SCALE = HD ** -0.5
TOL = {F32: 2e-4, BF16: 1.5e-2}
TOL_LSE = {F32: 1e-4, BF16: 5e-3}
KINK = 1e-4                       # px: the rule of tests/golden/kinks.py
ARENA = None
ERR_ARG = r"^%s failed: invalid argument$"
ERR_UNSUPPORTED = r"^%s failed: unsupported configuration$"
DN = {F32: "f32", BF16: "bf16"}

# (kind, dtype name, regime, output) -> (error measured on the CPU, bound = 4 x that); see the module docstring and tests/test_attn_edges_host.py.
# kind: "full" / "rvsa".  Only pairs whose measured error exceeds HALF the table value are listed; for every other pair the table holds.  Full attention:
# all seven are dq / dk in bf16: dS = P (dP - delta) is rounded to bf16 (2^-9 relative to each element) and delta is taken from the bf16-rounded o, while the sum
# dS K (dS^T Q) cancels -- the more, the more the softmax is peaked (R1 - R3) or the smaller q.k is against the bias terms (R4).
EXCEPTIONS = {
    ("full", "bf16", "R1", "dq"): (0.0129, 4 * 0.0129), ("full", "bf16", "R1", "dk"): (0.0132, 4 * 0.0132),
    ("full", "bf16", "R2", "dq"): (0.0199, 4 * 0.0199), ("full", "bf16", "R2", "dk"): (0.0207, 4 * 0.0207),
    ("full", "bf16", "R3", "dq"): (0.0168, 4 * 0.0168), ("full", "bf16", "R3", "dk"): (0.0180, 4 * 0.0180),
    ("full", "bf16", "R4", "dq"): (0.00828, 4 * 0.00828),
    # RVSA: the same, and the operands that are no inputs are rounded to bf16 too: the gathered K / V rows (bilinear blends) and the two relative-position
    # tables, whose product is taken with the UNSCALED q -- at logits of +-50 and |q . R| ~ 7 that moves a logit by some 0.03, a probability by 3 %.  In R2 the zero rows of padding and outside samples (logit ~ 0) take nearly all the weight from the real keys (logit ~ -45):
    # what is left of dq / dk and drel_h there is small and relatively coarse.
    ("rvsa", "bf16", "R0", "dk"): (0.00896, 4 * 0.00896),
    ("rvsa", "bf16", "R0", "dq"): (0.014, 4 * 0.014),
    ("rvsa", "bf16", "R1", "dk"): (0.0518, 4 * 0.0518),
    ("rvsa", "bf16", "R1", "dq"): (0.0492, 4 * 0.0492),
    ("rvsa", "bf16", "R1", "dv"): (0.0134, 4 * 0.0134),
    ("rvsa", "bf16", "R1", "o"): (0.0314, 4 * 0.0314),
    ("rvsa", "bf16", "R2", "dk"): (0.164, 4 * 0.164),
    ("rvsa", "bf16", "R2", "dq"): (0.175, 4 * 0.175),
    ("rvsa", "bf16", "R2", "drh"): (0.144, 4 * 0.144),
    ("rvsa", "bf16", "R2", "dv"): (0.0268, 4 * 0.0268),
    ("rvsa", "bf16", "R2", "o"): (0.0271, 4 * 0.0271),
    ("rvsa", "bf16", "R3", "dk"): (0.0213, 4 * 0.0213),
    ("rvsa", "bf16", "R3", "dq"): (0.0246, 4 * 0.0246),
    ("rvsa", "bf16", "R3", "dv"): (0.0104, 4 * 0.0104),
    ("rvsa", "bf16", "R3", "o"): (0.0182, 4 * 0.0182),
    ("rvsa", "bf16", "R4", "dk"): (0.0214, 4 * 0.0214),
    ("rvsa", "bf16", "R4", "dq"): (0.0239, 4 * 0.0239),
    ("rvsa", "bf16", "R4", "dv"): (0.00789, 4 * 0.00789),
    ("rvsa", "bf16", "R4", "o"): (0.00785, 4 * 0.00785),
    ("rvsa", "bf16", "R5m", "dk"): (0.0108, 4 * 0.0108),
    ("rvsa", "bf16", "R5m", "dq"): (0.0128, 4 * 0.0128),
}

# kernel families, by the names of mtp_amd.ops.FULL_FWD / FULL_BWD / RVSA_FWD / RVSA_BWD
FULL_GRIDS = {
    BF16: [((1, 1), "v3", "v3"), ((1, 2), "v3", "v3"), ((2, 1), "v3", "v3"), ((1, 16), "v3", "v3"), ((16, 1), "v3", "v3"), ((16, 16), "v3", "v3"),
           ((17, 16), "flash128", "flash"), ((16, 17), "flash128", "flash"),         # first flash grids: N = 272, key blocks that start mid-row
           ((26, 10), "flash128", "flash"),                                           # narrowest grid the flash backward takes
           ((29, 9), "flash128", "three_pass"), ((33, 8), "flash256", "three_pass"),  # Wp < 10: three-pass backward under a flash forward
           ((65, 4), "generic", "three_pass"), ((4, 65), "generic", "three_pass"),    # a side > 64
           ((17, 3), "generic", "single_wg")],                                        # <= 256 tokens but a table of 33 rows: the f32-math kernels in bf16
    F32: [((1, 1), "generic", "single_wg"), ((1, 2), "generic", "single_wg"), ((16, 16), "generic", "single_wg"),
          ((17, 16), "generic", "three_pass"), ((29, 9), "generic", "three_pass")],
}
RVSA_GRIDS = [(7, 7), (7, 8), (13, 7), (8, 8), (8, 9), (8, 13), (14, 7)]
RVSA_ATOMIC = {(8, 8), (8, 9)}           # mostly padding: nW * 24.5 > N
REGIMES = ["R0", "R1", "R2", "R3", "R4", "R4z"]
REGIMES_RVSA = REGIMES + ["R5", "R5m"]
BH = [(1, 1), (1, 3), (3, 1), (3, 3)]


def _thin(n_grids, regimes):
    """(grid index, B, heads, regime): every grid with every regime; the (B, heads) pair rotates, so each grid -- hence each family -- sees all four"""
    out = [(gi, *BH[(gi + ri) % 4], r) for gi in range(n_grids) for ri, r in enumerate(regimes)]
    for gi in range(n_grids):
        assert {(c[1], c[2]) for c in out if c[0] == gi} == set(BH)
    return out


def full_cases():
    return [(dt, g[0][0], g[0][1], B, heads, r, g[1], g[2]) for dt in (BF16, F32) for gi, B, heads, r in _thin(len(FULL_GRIDS[dt]), REGIMES)
            for g in [FULL_GRIDS[dt][gi]]]


def rvsa_cases():
    out = []
    for dt in (BF16, F32):
        for gi, B, heads, r in _thin(len(RVSA_GRIDS), REGIMES_RVSA):
            Hp, Wp = RVSA_GRIDS[gi]
            fb = "generic" if dt == F32 else ("mfma_atomic" if (Hp, Wp) in RVSA_ATOMIC else "mfma_dense")
            out.append((dt, Hp, Wp, B, heads, r, "generic" if dt == F32 else "mfma", fb))
    return out


def _id(c):
    return "%s-%dx%d-B%d-h%d-%s" % (DN[c[0]], c[1], c[2], c[3], c[4], c[5])


# ------------------------------------------------------------------------------------------------ inputs (CPU; shared with test_attn_edges_host.py)
def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rt(t, dtype):
    return t.to(dtype).float()


def _regime_qkv(qkv, do, rel, B, N, heads, regime, dtype):
    """applies the regime in place; returns the planted maxima [(image, query rows, key)]"""
    C = heads * HD
    v5 = qkv.view(B, N, 3, heads, HD)
    q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
    peaks = []
    if regime == "R1":
        q *= 4
        k *= 4
    elif regime in ("R2", "R3"):
        q.copy_(3 * q.abs())
        k.copy_((-3 if regime == "R2" else 3) * k.abs())
    elif regime in ("R4", "R4z"):
        qkv *= 0.25
        for t in rel:
            t *= (8.0 if regime == "R4" else 0.0)
    if B == 3:
        v[B - 1] /= 64
        do.view(B, N, C)[B - 1] /= 64
    qkv.copy_(_rt(qkv, dtype))
    return q, k, peaks


@functools.lru_cache(maxsize=None)
def full_case(dtype, Hp, Wp, B, heads, regime):
    N, C = Hp * Wp, heads * HD
    seed = 1000 * Hp + 10 * Wp + B + heads
    qkv, do = _rt(_rnd(B * N, 3 * C, seed=seed), dtype), _rt(_rnd(B * N, C, seed=seed + 3), dtype)
    rh, rw = 0.3 * _rnd(2 * Hp - 1, HD, seed=seed + 1), 0.3 * _rnd(2 * Wp - 1, HD, seed=seed + 2)
    q, k, peaks = _regime_qkv(qkv, do, (rh, rw), B, N, heads, regime, dtype)
    if regime == "R1":
        rows = [0] if N < 6 else [0, N // 3, N - 1]          # a minority of the rows: the slice's gradients keep their size
        for b, key in [(0, N - 1)] + ([(B - 1, 0)] if B > 1 else []):
            d = q[b, 0].clone()
            for r in rows:
                q[b, r] = d
            k[b, key] = 2 * d
            peaks.append((b, tuple(rows), key))
    return dict(qkv=qkv, do=do, rh=rh, rw=rw, peaks=peaks, B=B, Hp=Hp, Wp=Wp, heads=heads, N=N, C=C, dtype=dtype, regime=regime)


def full_eval(c, ref_dtype=torch.float64):
    """the oracle and its autograd gradients in ref_dtype: o, lse (B, heads, N), dqkv, drel_h, drel_w"""
    q = c["qkv"].to(ref_dtype).requires_grad_(True)
    rh, rw = c["rh"].to(ref_dtype).requires_grad_(True), c["rw"].to(ref_dtype).requires_grad_(True)
    o, lse = O.full_attn_fwd(q, c["B"], c["Hp"], c["Wp"], c["heads"], rh, rw, SCALE)
    gq, gh, gw = torch.autograd.grad(o, (q, rh, rw), c["do"].to(ref_dtype))
    return dict(o=o.detach(), lse=lse.detach(), dqkv=gq, drh=gh, drw=gw)


@functools.lru_cache(maxsize=None)
def full_ref(*key):
    return full_eval(full_case(*key))


def sample_coords(samp, B, Hp, Wp, heads):
    ix, iy = O.rvsa_sample_coords(samp.double(), B, Hp, Wp, heads)          # (B, heads, nh, nw, 7, 7)
    return ix, iy


def kink_distance(samp, B, Hp, Wp, heads):
    """per window (B * nh * nw): the smallest distance of any of its sample coordinates (all heads) to an integer, in px"""
    ix, iy = sample_coords(samp, B, Hp, Wp, heads)
    d = torch.minimum((ix - ix.round()).abs(), (iy - iy.round()).abs())
    return d.amin(dim=(4, 5)).amin(dim=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def rvsa_case(dtype, Hp, Wp, B, heads, regime):
    N, C = Hp * Wp, heads * HD
    nh, nw = (Hp + 6) // 7, (Wp + 6) // 7
    R = B * nh * nw
    seed = 2000 * Hp + 10 * Wp + B + heads
    qkv, do = _rt(_rnd(B * N, 3 * C, seed=seed), dtype), _rt(_rnd(B * N, C, seed=seed + 4), dtype)
    rh, rw, tab = 0.3 * _rnd(13, HD, seed=seed + 1), 0.3 * _rnd(13, HD, seed=seed + 2), 0.3 * _rnd(169, heads, seed=seed + 3)
    _regime_qkv(qkv, do, (rh, rw, tab), B, N, heads, regime, dtype)
    sscale = 3.0 if regime == "R5m" else 0.3
    for s in range(64):          # the first seed whose samples all keep KINK px from every integer (R5m: in at least 90 % of the windows, the others
                                 # are masked; R5: every sample is outside the map, where there is no kink to sit on)
        samp = sscale * _rnd(R, 5 * heads, seed=seed + 100 + s)
        if regime == "R5":
            samp[:, :2 * heads] = 50.0
        dist = kink_distance(samp, B, Hp, Wp, heads)
        if regime == "R5" or float(dist.min()) >= KINK or (regime == "R5m" and float((dist >= KINK).double().mean()) >= 0.9):
            break
    else:
        raise AssertionError("no kink-free sampling seed")
    return dict(qkv=qkv, do=do, rh=rh, rw=rw, tab=tab, samp=samp, B=B, Hp=Hp, Wp=Wp, heads=heads, N=N, C=C, nh=nh, nw=nw, R=R, dtype=dtype, regime=regime)


def rvsa_eval(c, ref_dtype=torch.float64):
    q, sp = c["qkv"].to(ref_dtype).requires_grad_(True), c["samp"].to(ref_dtype).requires_grad_(True)
    rh, rw, tab = (c[n].to(ref_dtype).requires_grad_(True) for n in ("rh", "rw", "tab"))
    o, lse = O.rvsa_attn_fwd(q, sp, c["B"], c["Hp"], c["Wp"], c["heads"], rh, rw, tab, SCALE)        # lse (B, heads, nh, nw, 49)
    gq, gs, gh, gw, gt = torch.autograd.grad(o, (q, sp, rh, rw, tab), c["do"].to(ref_dtype), allow_unused=True)
    gs = torch.zeros_like(sp) if gs is None else gs
    return dict(o=o.detach(), lse=lse.detach().reshape(c["B"], c["heads"], -1), dqkv=gq, dsamp=gs, drh=gh, drw=gw, dtab=gt)


@functools.lru_cache(maxsize=None)
def rvsa_ref(*key):
    return rvsa_eval(rvsa_case(*key))


# ------------------------------------------------------------------------------------------------ errors and bounds
def slice_err(got, ref, B, heads, floor=None):
    """max over the (image, head) slices of max |got - ref| / max(max |ref|, floor); got / ref (B * N, heads * w) or (B, heads, n)"""
    got, ref = got.double(), ref.double()
    if got.dim() == 2:
        got, ref = (t.reshape(B, -1, heads, t.shape[1] // heads).permute(0, 2, 1, 3).reshape(B, heads, -1) for t in (got, ref))
    den = ref.abs().amax(-1)
    if floor is not None:
        den = torch.maximum(den, torch.as_tensor(floor, dtype=den.dtype).expand_as(den))
    dif = (got - ref).abs().amax(-1)
    err = torch.where(den > 0, dif / den, torch.where(dif == 0, torch.zeros_like(dif), torch.full_like(dif, float("inf"))))
    return float(err.nan_to_num(float("inf")).max())


def tiny_grid_floor(c):
    """(B, heads) scale of the terms of dq / dk on a grid of one or two tokens (see the module docstring)"""
    B, heads, N = c["B"], c["heads"], c["N"]
    qkv = c["qkv"].double().reshape(B, N, 3, heads, HD)
    terms = (c["do"].double().reshape(B, N, heads, HD).abs().amax(1) * qkv[:, :, 2].abs().amax(1)).sum(-1)
    return terms * qkv[:, :, :2].abs().amax(dim=(1, 2, 4)) * SCALE


def table_err(got, ref, other_ref, rows, floor=0.0):
    """whole-tensor; a one-row table is measured against the other table's gradient, and on a grid of two tokens both against at least the scale of
    the terms (the floor of dq / dk, summed over the slices: the table gradients are sums of the same dS over all of them)"""
    den = float(ref.double().abs().max()) if rows > 1 else float(other_ref.double().abs().max())
    return float((got.double() - ref.double()).abs().max()) / (max(den, floor) + 1e-30)


def errors(c, ref, got, rvsa):
    """{output: (error, kind of bound)} for o, lse, dq, dk, dv, the table gradients and dsamp"""
    B, heads, C = c["B"], c["heads"], c["C"]
    fl = tiny_grid_floor(c) if (not rvsa and c["N"] <= 2) else None
    out = {"o": (slice_err(got["o"], ref["o"], B, heads), "out"),
           "lse": (slice_err(got["lse"].reshape(B, heads, -1), ref["lse"], B, heads, floor=1.0), "lse"),
           "dq": (slice_err(got["dqkv"][:, :C], ref["dqkv"][:, :C], B, heads, floor=fl), "out"),
           "dk": (slice_err(got["dqkv"][:, C:2 * C], ref["dqkv"][:, C:2 * C], B, heads, floor=fl), "out"),
           "dv": (slice_err(got["dqkv"][:, 2 * C:], ref["dqkv"][:, 2 * C:], B, heads), "out")}
    if not (not rvsa and c["N"] == 1):                 # (one token: both table gradients are exactly zero, like dq and dk)
        tf = float(fl.sum()) if fl is not None else 0.0
        out["drh"] = (table_err(got["drh"], ref["drh"], ref["drw"], ref["drh"].shape[0], tf), "tab")
        out["drw"] = (table_err(got["drw"], ref["drw"], ref["drh"], ref["drw"].shape[0], tf), "tab")
    if rvsa:
        out["dtab"] = (rel_err(got["dtab"], ref["dtab"]), "tab")
    return out


def bound(kind, dtype, regime, name, what):
    ex = EXCEPTIONS.get((kind, DN[dtype], regime, name))
    if ex is not None:
        return ex[1]
    return {"out": TOL[dtype], "lse": TOL_LSE[dtype], "tab": 10 * TOL[dtype]}[what]


def check_errors(kind, family, c, errs):
    dtype, regime = c["dtype"], c["regime"]
    tag = "%s_%dx%d_B%d_h%d" % (DN[dtype], c["Hp"], c["Wp"], c["B"], c["heads"])
    bad = []
    for name, (err, what) in errs.items():
        record_parity("attn_edges_%s_%s" % (family, regime), "%s_%s" % (name, tag), err)
        b = bound(kind, dtype, regime, name, what)
        print("attn_edges %s %s %s %s: err %.3g bound %.3g" % (family, regime, tag, name, err, b))
        if not err <= b:
            bad.append("%s: %.3g > %.3g" % (name, err, b))
    assert not bad, "%s %s %s: %s" % (family, regime, tag, "; ".join(bad))


# ------------------------------------------------------------------------------------------------ fixtures
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
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t):
    return ARENA.like(t)


def e(*shape, dtype=F32):
    return ARENA.empty(*shape, dtype=dtype)


def gpu_full(ops, c, qkv=None, do=None, **bw):
    """forward + backward on fresh guarded buffers; returns CPU tensors (floats of the op's dtype)"""
    dtype, B, Hp, Wp, heads, N, C = (c[n] for n in ("dtype", "B", "Hp", "Wp", "heads", "N", "C"))
    qd, dod, rh, rw = dev(c["qkv"] if qkv is None else qkv, dtype), dev(c["do"] if do is None else do, dtype), dev(c["rh"]), dev(c["rw"])
    o, lse = e(B * N, C, dtype=dtype), e(B * heads * N)
    ops.full_attn_fwd(qd, o, lse, rh, rw, B, Hp, Wp, heads, SCALE)
    dqkv, drh, drw = e(B * N, 3 * C, dtype=dtype), e(2 * Hp - 1, HD), e(2 * Wp - 1, HD)
    ops.full_attn_bwd(qd, ARENA.frozen(o), dod, ARENA.frozen(lse), dqkv, rh, rw, drh, drw, B, Hp, Wp, heads, SCALE, **bw)
    return dict(o=o.float().cpu(), lse=lse.cpu(), dqkv=dqkv.float().cpu(), drh=drh.cpu(), drw=drw.cpu())


def gpu_rvsa(ops, c, qkv=None, do=None, samp=None):
    dtype, B, Hp, Wp, heads, N, C, R = (c[n] for n in ("dtype", "B", "Hp", "Wp", "heads", "N", "C", "R"))
    qd, dod, sd = dev(c["qkv"] if qkv is None else qkv, dtype), dev(c["do"] if do is None else do, dtype), dev(c["samp"] if samp is None else samp)
    rh, rw, tab = dev(c["rh"]), dev(c["rw"]), dev(c["tab"])
    o, lse = e(B * N, C, dtype=dtype), e(R * heads * 49)
    ops.rvsa_attn_fwd(qd, sd, o, lse, rh, rw, tab, B, Hp, Wp, heads, SCALE)
    dqkv, dsamp, drh, drw, dtab = e(B * N, 3 * C, dtype=dtype), e(R, 5 * heads), e(13, HD), e(13, HD), e(169, heads)
    ops.rvsa_attn_bwd(qd, sd, ARENA.frozen(o), dod, ARENA.frozen(lse), dqkv, dsamp, rh, rw, tab, drh, drw, dtab, B, Hp, Wp, heads, SCALE)
    lse_bh = lse.cpu().reshape(B, c["nh"] * c["nw"], heads, 49).permute(0, 2, 1, 3).reshape(B, heads, -1)       # as the oracle orders it
    return dict(o=o.float().cpu(), lse=lse_bh, dqkv=dqkv.float().cpu(), dsamp=dsamp.cpu(), drh=drh.cpu(), drw=drw.cpu(), dtab=dtab.cpu())


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("case", full_cases(), ids=_id)
def test_full_attention_regimes_at_the_smallest_grid_of_each_family(ops, case):
    dtype, Hp, Wp, B, heads, regime, ff, fb = case
    assert ops.full_attn_kernel(dtype, Hp, Wp) == ops.FULL_FWD[ff] and ops.full_attn_kernel(dtype, Hp, Wp, backward=True) == ops.FULL_BWD[fb]
    key = case[:6]
    c, ref = full_case(*key), full_ref(*key)
    got = gpu_full(ops, c)
    check_errors("full", "full_%s_%s" % (ff, fb), c, errors(c, ref, got, False))


@pytest.mark.parametrize("case", rvsa_cases(), ids=_id)
def test_rvsa_attention_regimes_at_the_smallest_grids(ops, case):
    """dsamp is compared in full (the sampling seeds keep every sample KINK px from an integer: test_attn_edges_host.py asserts it), except in R5
    (every sample outside the map: o, the dk / dv parts of dqkv and dsamp are EXACTLY zero, lse is the logsumexp of the bias terms) and R5m
    (3 randn sampling: only windows whose samples all keep KINK px from an integer)"""
    dtype, Hp, Wp, B, heads, regime, ff, fb = case
    assert ops.rvsa_attn_kernel(dtype, Hp, Wp, heads) == ops.RVSA_FWD[ff] and ops.rvsa_attn_kernel(dtype, Hp, Wp, heads, backward=True) == ops.RVSA_BWD[fb]
    key = case[:6]
    c, ref = rvsa_case(*key), rvsa_ref(*key)
    got = gpu_rvsa(ops, c)
    C = c["C"]
    family = "rvsa_%s_%s" % (ff, fb)
    if regime == "R5":
        assert float(ref["o"].abs().max()) == 0.0 and float(ref["dsamp"].abs().max()) == 0.0
        for name, t in (("o", got["o"]), ("dk dv", got["dqkv"][:, C:]), ("dsamp", got["dsamp"])):
            assert float(t.abs().max()) == 0.0, "%s must be exactly zero when every sample lies outside the map" % name
        errs = errors(c, ref, got, True)
        errs = {n: errs[n] for n in ("lse", "dq", "drh", "drw", "dtab")}
    else:
        errs = errors(c, ref, got, True)
        if regime == "R5m":
            ok = kink_distance(c["samp"], B, Hp, Wp, heads) >= KINK
            errs["dsamp"] = (rel_err(got["dsamp"][ok], ref["dsamp"][ok]), "tab")
        else:
            errs["dsamp"] = (rel_err(got["dsamp"], ref["dsamp"]), "tab")
    check_errors("rvsa", family, c, errs)


# ------------------------------------------------------------------------------------------------ isolation between images
def _bits(t):
    return t.contiguous().view(torch.int32)


def _images_equal(t, B, what, only=None):
    t = t.reshape(B, -1)
    for b in (only or range(1, B)):
        assert torch.equal(_bits(t[0]), _bits(t[b])), "%s: image %d differs from image 0" % (what, b)


ISO_FULL = [(BF16, 9, 12), (BF16, 17, 16), (BF16, 29, 9), (BF16, 33, 8), (BF16, 65, 4), (BF16, 17, 3), (F32, 9, 12), (F32, 17, 16)]
ISO_RVSA = [(BF16, 7, 8), (BF16, 8, 8), (F32, 7, 8)]


@pytest.mark.parametrize("dtype,Hp,Wp", ISO_FULL, ids=lambda v: DN.get(v, str(v)))
def test_full_attention_images_do_not_see_each_other(ops, dtype, Hp, Wp):
    """one image replicated three times: the three slices of o, lse and dqkv are bit-identical; then image 1's qkv and dout alone change: slices 0 and 2
    keep every bit"""
    c1 = full_case(dtype, Hp, Wp, 1, 2, "R0")
    c = dict(c1, B=3, qkv=c1["qkv"].repeat(3, 1), do=c1["do"].repeat(3, 1))
    a = gpu_full(ops, c)
    for n in ("o", "lse", "dqkv"):
        _images_equal(a[n], 3, n)
    other = full_case(dtype, Hp, Wp, 1, 2, "R3")
    qkv2, do2 = c["qkv"].clone(), c["do"].clone()
    qkv2.view(3, -1)[1], do2.view(3, -1)[1] = other["qkv"].reshape(-1), -other["do"].reshape(-1)
    b = gpu_full(ops, c, qkv=qkv2, do=do2)
    for n in ("o", "lse", "dqkv"):
        x, y = a[n].reshape(3, -1), b[n].reshape(3, -1)
        assert torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[2]), _bits(y[2])), n
        assert not torch.equal(_bits(x[1]), _bits(y[1])), n


@pytest.mark.parametrize("dtype,Hp,Wp", ISO_RVSA, ids=lambda v: DN.get(v, str(v)))
def test_rvsa_attention_images_do_not_see_each_other(ops, dtype, Hp, Wp):
    """as above, with dsamp.  The bit-identity of the dk / dv part of dqkv is skipped -- there and only there -- where the k / v gradients are scattered by
    f32 atomics, whose order is not fixed: the atomic-scatter backward (bf16 8 x 8) and the generic f32 kernel; the values are still held to the table."""
    c1 = rvsa_case(dtype, Hp, Wp, 1, 2, "R0")
    rep = lambda t: t.repeat(3, 1)
    c = dict(c1, B=3, R=3 * c1["R"], qkv=rep(c1["qkv"]), do=rep(c1["do"]), samp=rep(c1["samp"]))
    atomic = ops.rvsa_attn_kernel(dtype, Hp, Wp, 2, backward=True) != ops.RVSA_BWD["mfma_dense"]
    C = c["C"]

    def parts(r):
        d = {"o": r["o"], "lse": r["lse"], "dq": r["dqkv"][:, :C], "dsamp": r["dsamp"]}
        if not atomic:
            d["dkv"] = r["dqkv"][:, C:]
        return d
    a = gpu_rvsa(ops, c)
    pa = parts(a)
    for n, t in pa.items():
        _images_equal(t, 3, n)
    if atomic:
        x = a["dqkv"][:, C:].reshape(3, -1)
        assert rel_err(x[1], x[0]) < TOL[dtype] and rel_err(x[2], x[0]) < TOL[dtype]
    other = rvsa_case(dtype, Hp, Wp, 1, 2, "R3")
    qkv2, do2 = c["qkv"].clone(), c["do"].clone()
    qkv2.view(3, -1)[1], do2.view(3, -1)[1] = other["qkv"].reshape(-1), -other["do"].reshape(-1)
    pb = parts(gpu_rvsa(ops, c, qkv=qkv2, do=do2))
    for n in pa:
        x, y = pa[n].reshape(3, -1), pb[n].reshape(3, -1)
        assert torch.equal(_bits(x[0]), _bits(y[0])) and torch.equal(_bits(x[2]), _bits(y[2])), n
        assert not torch.equal(_bits(x[1]), _bits(y[1])), n


# ------------------------------------------------------------------------------------------------ the wrappers' accumulate / defer paths
def _pair(n0, n1, adjacent, base=None):
    """two f32 gradient buffers of n0 and n1 floats: adjacent halves of one guarded buffer, or two buffers"""
    if adjacent:
        buf = io(base) if base is not None else e(n0 + n1)
        return buf[:n0], buf[n0:]
    return (io(base[:n0]), io(base[n0:])) if base is not None else (e(n0), e(n1))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Hp,Wp", [(9, 12), (17, 16)])
def test_full_attn_bwd_accumulate_and_deferred_reduction(ops, dtype, Hp, Wp):
    key = (dtype, Hp, Wp, 3, 2, "R0")
    c, ref = full_case(*key), full_ref(*key)
    B, heads, N, C = 3, 2, c["N"], c["C"]
    nh_, nw_ = (2 * Hp - 1) * HD, (2 * Wp - 1) * HD
    qd, dod, rh, rw = dev(c["qkv"], dtype), dev(c["do"], dtype), dev(c["rh"]), dev(c["rw"])
    o, lse = e(B * N, C, dtype=dtype), e(B * heads * N)
    ops.full_attn_fwd(qd, o, lse, rh, rw, B, Hp, Wp, heads, SCALE)

    def bwd(drh, drw, **kw):
        ops.full_attn_bwd(qd, o, dod, lse, e(B * N, 3 * C, dtype=dtype), rh, rw, drh.view(-1, HD), drw.view(-1, HD), B, Hp, Wp, heads, SCALE, **kw)
    now_h, now_w = _pair(nh_, nw_, False)
    bwd(now_h, now_w)                                                    # the immediate path, separate buffers
    assert rel_err(now_h.cpu(), ref["drh"].reshape(-1)) < 10 * TOL[dtype] and rel_err(now_w.cpu(), ref["drw"].reshape(-1)) < 10 * TOL[dtype]
    base = _rnd(nh_ + nw_, seed=5)
    for adjacent in (False, True):                                       # accumulate onto a non-zero base, two launches resp. one
        ah, aw = _pair(nh_, nw_, adjacent, base)
        bwd(ah, aw, accumulate=True)
        want = base.double() + torch.cat([ref["drh"].reshape(-1), ref["drw"].reshape(-1)])
        assert rel_err(torch.cat([ah, aw]).cpu(), want) < 10 * TOL[dtype]
    for acc in (False, True):                                            # deferred: adjacent halves of one buffer, reduced later
        dh, dw = _pair(nh_, nw_, True, base if acc else None)
        items = []
        bwd(dh, dw, accumulate=acc, defer=items)
        assert len(items) == 1
        ops.reduce_rows_deferred(items)
        assert items == []
        want = torch.cat([now_h, now_w]).cpu().double() + (base.double() if acc else 0)
        assert rel_err(torch.cat([dh, dw]).cpu(), want) < 1e-6
    sh, sw = _pair(nh_, nw_, False)                                      # not adjacent: reduced at once, nothing queued
    items = []
    bwd(sh, sw, defer=items)
    assert items == [] and rel_err(sh.cpu(), now_h.cpu()) < 1e-6 and rel_err(sw.cpu(), now_w.cpu()) < 1e-6


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Hp,Wp", [(7, 8), (8, 8)])
def test_rvsa_attn_bwd_accumulate_and_deferred_reduction(ops, dtype, Hp, Wp):
    key = (dtype, Hp, Wp, 3, 2, "R0")
    c, ref = rvsa_case(*key), rvsa_ref(*key)
    B, heads, N, C, R = 3, 2, c["N"], c["C"], c["R"]
    n13 = 13 * HD
    qd, dod, sd, rh, rw, tab = dev(c["qkv"], dtype), dev(c["do"], dtype), dev(c["samp"]), dev(c["rh"]), dev(c["rw"]), dev(c["tab"])
    o, lse = e(B * N, C, dtype=dtype), e(R * heads * 49)
    ops.rvsa_attn_fwd(qd, sd, o, lse, rh, rw, tab, B, Hp, Wp, heads, SCALE)

    def bwd(drh, drw, dtab, **kw):
        ops.rvsa_attn_bwd(qd, sd, o, dod, lse, e(B * N, 3 * C, dtype=dtype), e(R, 5 * heads), rh, rw, tab, drh.view(13, HD), drw.view(13, HD), dtab,
                          B, Hp, Wp, heads, SCALE, **kw)
    now_h, now_w = _pair(n13, n13, False)
    now_t = e(169, heads)
    bwd(now_h, now_w, now_t)
    for got, name in ((now_h, "drh"), (now_w, "drw"), (now_t, "dtab")):
        assert rel_err(got.cpu().reshape(-1), ref[name].reshape(-1)) < 10 * TOL[dtype], name
    base, base_t = _rnd(2 * n13, seed=6), _rnd(169, heads, seed=7)
    for adjacent in (False, True):
        ah, aw = _pair(n13, n13, adjacent, base)
        at = io(base_t)
        bwd(ah, aw, at, accumulate=True)
        assert rel_err(torch.cat([ah, aw]).cpu(), base.double() + torch.cat([ref["drh"].reshape(-1), ref["drw"].reshape(-1)])) < 10 * TOL[dtype]
        assert rel_err(at.cpu(), base_t.double() + ref["dtab"]) < 10 * TOL[dtype]
    for acc in (False, True):
        dh, dw = _pair(n13, n13, True, base if acc else None)
        dt_ = io(base_t) if acc else e(169, heads)
        items = []
        bwd(dh, dw, dt_, accumulate=acc, defer=items)
        assert len(items) == 2                                           # the drel_h | drel_w pair and the transposed (heads, 169) table partials
        ops.reduce_rows_deferred(items)
        assert items == []
        assert rel_err(torch.cat([dh, dw]).cpu(), torch.cat([now_h, now_w]).cpu().double() + (base.double() if acc else 0)) < 1e-6
        assert rel_err(dt_.cpu(), now_t.cpu().double() + (base_t.double() if acc else 0)) < 1e-6
    sh, sw = _pair(n13, n13, False)
    st, items = e(169, heads), []
    bwd(sh, sw, st, defer=items)
    assert items == [] and rel_err(sh.cpu(), now_h.cpu()) < 1e-6 and rel_err(sw.cpu(), now_w.cpu()) < 1e-6 and rel_err(st.cpu(), now_t.cpu()) < 1e-6


# ------------------------------------------------------------------------------------------------ refusals
def test_attention_refusals_leave_every_output_untouched(ops):
    """each refusal comes back from the argument / configuration checks, before any launch: the exact _lib.check text, every output still poison"""
    heads, B = 2, 1

    def full(dtype, Hp, Wp, hd=HD, B_arg=None, Hb=None, fwd=True, bwd=True, err=ERR_ARG):
        Hs, Ws = max(Hp, 1), max(Wp, 1)
        T, C = B * Hs * Ws, heads * hd
        qkv, do = dev(_rnd(T, 3 * C, seed=1), dtype), dev(_rnd(T, C, seed=2), dtype)
        rh, rw = dev(_rnd(2 * Hs - 1, hd, seed=3)), dev(_rnd(2 * Ws - 1, hd, seed=4))
        o, lse = ARENA.wide(T, C, dtype=dtype), ARENA.wide(1, B * heads * Hs * Ws)
        dqkv, drh, drw = ARENA.wide(T, 3 * C, dtype=dtype), ARENA.wide(2 * Hs - 1, hd), ARENA.wide(2 * Ws - 1, hd)
        Ba = B if B_arg is None else B_arg
        if fwd:
            with pytest.raises(RuntimeError, match=err % "mtp_full_attn_fwd"):
                ops.full_attn_fwd(qkv, o, lse.view(-1), rh, rw, Ba, Hp, Wp, heads, SCALE)
        if bwd:
            with pytest.raises(RuntimeError, match=err % "mtp_full_attn_bwd"):
                ops.full_attn_bwd(qkv, dev(_rnd(T, C, seed=5), dtype), do, dev(_rnd(B * heads * Hs * Ws, seed=6)), dqkv, rh, rw, drh, drw, Ba, Hp, Wp, heads, SCALE)

    def rvsa(dtype, Hp, Wp, hd=HD, B_arg=None, err=ERR_ARG):
        Hs, Ws = max(Hp, 7), max(Wp, 7)
        nh, nw = ops.rvsa_windows(Hs, Ws)
        T, C, R = B * Hs * Ws, heads * hd, B * nh * nw
        qkv, do, samp = dev(_rnd(T, 3 * C, seed=1), dtype), dev(_rnd(T, C, seed=2), dtype), dev(0.3 * _rnd(R, 5 * heads, seed=3))
        rh, rw, tab = dev(_rnd(13, hd, seed=4)), dev(_rnd(13, hd, seed=5)), dev(_rnd(169, heads, seed=6))
        o, lse = ARENA.wide(T, C, dtype=dtype), ARENA.wide(1, R * heads * 49)
        dqkv, dsamp, drh, drw, dtab = ARENA.wide(T, 3 * C, dtype=dtype), ARENA.wide(R, 5 * heads), ARENA.wide(13, hd), ARENA.wide(13, hd), ARENA.wide(169, heads)
        Ba = B if B_arg is None else B_arg
        with pytest.raises(RuntimeError, match=err % "mtp_rvsa_attn_fwd"):
            ops.rvsa_attn_fwd(qkv, samp, o, lse.view(-1), rh, rw, tab, Ba, Hp, Wp, heads, SCALE)
        with pytest.raises(RuntimeError, match=err % "mtp_rvsa_attn_bwd"):
            ops.rvsa_attn_bwd(qkv, samp, dev(_rnd(T, C, seed=7), dtype), do, dev(_rnd(R * heads * 49, seed=8)), dqkv, dsamp, rh, rw, tab, drh, drw, dtab,
                              Ba, Hp, Wp, heads, SCALE)
    for dtype in (F32, BF16):
        full(dtype, 3, 4, hd=32, err=ERR_UNSUPPORTED)                   # head_dim != 64
        rvsa(dtype, 7, 8, hd=32, err=ERR_UNSUPPORTED)
        rvsa(dtype, 6, 8)                                               # a side below one window
        rvsa(dtype, 8, 6)
        full(dtype, 3, 4, B_arg=0)
        rvsa(dtype, 7, 8, B_arg=0)
        full(dtype, 0, 4)                                               # Hp = 0: the forward and (since this change) the backward
        full(dtype, 4, 0)
    full(BF16, 1, 257, err=ERR_UNSUPPORTED, bwd=False)                  # the f32-math forward's LDS need exceeds 160 KiB and no MFMA family takes the grid
    assert ops.full_attn_kernel(BF16, 1, 257) == 0
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_full_attn_kernel"):
        ops.full_attn_kernel(BF16, 0, 4)
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_rvsa_attn_kernel"):
        ops.rvsa_attn_kernel(BF16, 6, 8, 2)
    torch.cuda.synchronize()
    ARENA.check()
