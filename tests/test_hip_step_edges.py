"""GPU: the optimizer step (csrc/optimizer.hip) and the step glue around it at their seams, every buffer out of the guard arena (tests/guard.py): outputs
NaN-poisoned and between guards, inputs frozen, buffers updated in place between guards, the wrappers' workspaces poisoned and guarded.

* Sums (mtp_sqnorm_f32, mtp_sqnorm_segments_f32, mtp_colsum[_acc], mtp_reduce_rows_t[_batched]_f32) get optim_ref.exact_ints -- values in {-1, 0, 1}, whose
  partial sums are integers in any order -- and must return THE integer: a dropped or doubled element is a wrong answer, not an error inside a tolerance.
* Data movement (zero / copy segments, patchify, ConvTranspose packing, weight images, split-K partial sums) is compared bit for bit.
* AdamW (mtp_adamw_flat[_lr], mtp_adamw_weight_images[_lr]) is compared step by step with optim_ref.adamw_ref -- the same update in float64 from the state the
  kernel started from -- under element-wise bounds:

      m' = b1 m + (1 - b1) ge,  v' = b2 v + (1 - b2) ge ge,  ge = g gs,  gs = grad_scale min(1, max_norm / (sqrt(sqn) grad_scale + 1e-6))

  counted in units of 2^-24 (one correctly rounded f32 operation; sqrtf and the division, which need only be good to 1 ulp, count 2):
  gs: sqrtf 2, x grad_scale 1, + 1e-6 1, max_norm / 2, x coef 1 = 7;  ge = g gs: 8;  (1 - b1 and 1 - b2 are exact: Sterbenz)
  m': (1 - b1) ge 9, the sum 10, against 2 on the b1 m term  ->  |m' - ref| <= 10 x 2^-24 (|b1 m| + |(1 - b1) ge|): M_K = 11 with the second-order terms
  v': (1 - b2) ge 9, x ge 9 + 8 + 1 = 18, the sum 19          ->  |v' - ref| <= 19 x 2^-24 (|b2 v| + |(1 - b2) ge^2|): V_K = 20 likewise
  (a fused multiply-add in place of a multiply and an add only removes a rounding).

  p' = p (1 - lr wd) - (lr / bc1) m' / (sqrtf(v') rsqrtf(bc2) + eps) runs through sqrtf, rsqrtf and a division whose errors nothing in the project fixes, so
  its bound is measured: the worst |p' - ref| / (2^-24 (|p| + |update|)) over every regime, layout and entry point below (P_MEASURED), times 4 for other
  seeds (a handful of roundings, not a data-dependent accumulation).  Every run records its ratio (conftest.record_parity, group "step_edges")."""
import ctypes as C

import pytest
import torch

import guard
import optim_ref as R
from conftest import record_parity
from oracle import vit_rvsa_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
ARENA = None     # the running test's guard.Arena
ERR_ARG = r"^%s failed: invalid argument$"      # what _lib.check raises for MTP_ERR_ARG (-1) and for nothing else
U = 2.0 ** -24
M_K, V_K = 11, 20
P_MEASURED = 3.31        # worst ratio on an MI355X: mtp_adamw_flat, clipping, the 8 M element case (3.3007); seam layout 2.60, zero gradient 1.48
P_K = 4 * P_MEASURED


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


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape) + 7 * len(shape))
    t = torch.randn(*shape, generator=g) * scale
    return t.to(dtype).float() if dtype == BF16 else t    # values exactly representable in the op's dtype


def dev(t, dtype=None):
    """an op INPUT: guarded and frozen"""
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def io(t, dtype=None):
    """updated in place by contract: guarded, not frozen"""
    return ARENA.like(t, dtype=dtype or t.dtype)


def e(*shape, dtype=F32):
    """an op OUTPUT: NaN-poisoned, between guards"""
    return ARENA.empty(*shape, dtype=dtype)


def within(got, ref, bound, what=""):
    """element-wise |got - ref| <= bound, all in float64; NaN (a never-written element) fails"""
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), "%s: %d of %d elements outside the bound; worst |err| / bound = %.3g at %s" % (
        what, int((~ok).sum()), ok.numel(), float((err / bound.clamp_min(1e-300))[~ok].nan_to_num(float("inf")).max()), tuple((~ok).nonzero()[0].tolist()))


def bits(t):
    return t.contiguous().view(torch.int32)


def i64(values):
    return dev(torch.tensor(values, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ squared norms, clearing
@pytest.mark.parametrize("n", R.SQNORM_SIZES)
def test_sqnorm_returns_the_integer(ops, n):
    """below one float4 (the tail alone), the tail next to whole float4s, around one workgroup's 1024 elements, and 2048 workgroups' worth plus 5: the
    grid-stride loop and the tail in one launch.  A second call adds the same integer again (out +=)"""
    x = R.exact_ints(n, seed=1)
    x[-3:] = torch.tensor([1.0, -1.0, 1.0])[-min(n, 3):]          # whatever the tail holds counts
    want = int((x != 0).sum())
    dx, out = dev(x), ARENA.zeros(1)
    ops.sqnorm(dx, out)
    assert out.item() == want
    ops.sqnorm(dx, out)
    assert out.item() == 2 * want < 2 ** 24


def _tables():
    """name -> [(start, count)]: disjoint runs inside a base buffer of R.SEGMENT_BASE floats"""
    mixed, cur = [], 0
    # 16-byte-aligned runs, odd starts, odd counts, one element, and the host's piece sizes 8191 / 8192 / 65536 -- aligned and not
    for start_off, count in [(0, 4), (0, 256), (1, 8), (0, 7), (3, 1), (0, 8191), (0, 8192), (0, 65536), (2, 65536), (1, 8191), (0, 1), (0, 12), (3, 5), (0, 1028)]:
        cur = (cur + 3) // 4 * 4 + start_off
        mixed.append((cur, count))
        cur += count + 1
    assert cur <= R.SEGMENT_BASE
    many = [(8 * i + (i % 2) + (i % 3 == 0), 1 + (i + 1) % 6) for i in range(4097)]  # 8-float slots: starts of residue 0, 1, 2 and counts 1 .. 6, aligned runs among them
    assert any(s % 4 == 0 and c % 4 == 0 for s, c in many) and any(s % 4 and c % 4 for s, c in many) and any(s % 4 == 0 and c % 4 for s, c in many)
    assert all(s + c <= 8 * i + 8 for i, (s, c) in enumerate(many))
    return {"mixed": mixed, "one": [(4, 65536)], "one_odd": [(5, 3)], "4096": many[:4096], "4097": many}


@pytest.mark.parametrize("table", ["mixed", "one", "one_odd", "4096", "4097"])
def test_sqnorm_segments_returns_the_integer_on_top_of_its_start_value(ops, table):
    """the launch has at most 4096 workgroups: 4097 runs make the first one take a second run"""
    runs = _tables()[table]
    base = R.exact_ints(R.SEGMENT_BASE, seed=2)
    want = sum(int((base[s:s + c] != 0).sum()) for s, c in runs)
    assert want > 0
    db, start, count = dev(base), i64([s for s, _ in runs]), i64([c for _, c in runs])
    out = io(torch.tensor([7.0]))
    ops.sqnorm_segments(db, start, count, out)
    assert out.item() == 7 + want
    ops.sqnorm_segments(db, start, count, out)
    assert out.item() == 7 + 2 * want < 2 ** 24


@pytest.mark.parametrize("table", ["mixed", "one", "one_odd", "4096", "4097"])
def test_zero_segments_clears_the_listed_runs_and_nothing_else(ops, table):
    runs = _tables()[table]
    base = torch.full((R.SEGMENT_BASE,), -3.25)
    want = base.clone()
    for s, c in runs:
        want[s:s + c] = 0.0
    db = io(base)
    ops.zero_segments(db, i64([s for s, _ in runs]), i64([c for _, c in runs]))
    assert torch.equal(bits(db.cpu()), bits(want))


# ------------------------------------------------------------------------------------------------ AdamW
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
KINDS = {"flat": ("flat", BF16), "images": ("images", BF16), "images_f32": ("images", F32)}
LAYOUTS = {"seam": R.SEAM_SHAPES, "single": [((72, 68), True, True, True)]}
LR_ZERO_SEG = 8          # (68, 72) between the 1-D parameters of 64 and 65 elements
# sqn: "true" = the squared norm of the step's gradient; +1 / -1 = the value that puts sqrt(sqn) grad_scale at max_norm (1 +- 2^-10); None = no clipping
REGIMES = {
    "clip": dict(sqn="true", max_norm=1.0, gs=1.0),
    "edge_above": dict(sqn=+1, max_norm=5.0, gs=1.0),
    "edge_below": dict(sqn=-1, max_norm=5.0, gs=1.0),
    "no_norm": dict(sqn=None, max_norm=5.0, gs=0.5),
    "gs8_clip": dict(sqn="true", max_norm=1.0, gs=0.125),
    "gs8_noclip": dict(sqn="true", max_norm=1e4, gs=0.125),
    "zero_grad": dict(sqn="true", max_norm=5.0, gs=1.0, g=0.0, steps=1),
    "late_tiny": dict(sqn=None, max_norm=0.0, gs=1.0, g=1e-12, late=True),
    "late_huge": dict(sqn=None, max_norm=0.0, gs=1.0, g=1e12, late=True),
    "lr_zero": dict(sqn="true", max_norm=1.0, gs=1.0, lr_zero=LR_ZERO_SEG),
}
FORMS = ["lr", "plain"]
CASES = [(k, f, r) for r in REGIMES for k in KINDS for f in FORMS if not (r == "lr_zero" and f == "plain")]
_DONE = {}


def _seg_params(n, lr_zero=None):
    """every segment its own weight decay and lr scale (f32 values); every fourth one has no weight decay"""
    wd = torch.tensor([0.0 if i % 4 == 1 else 0.01 * (i + 1) for i in range(n)])
    sc = torch.tensor([1.0 / (1.0 + 0.07 * i) for i in range(n)])
    if lr_zero is not None:
        sc[lr_zero] = 0.0
    return wd, sc


def _adamw_launch(ops, kind, plain, st, hyper, sqn, max_norm, gs):
    if KINDS[kind][0] == "flat":
        if plain:
            ops.adamw_flat(st["p"], st["g"], st["m"], st["v"], st["seg_start"], st["seg_wd"], hyper, sqn, max_norm, gs)
        else:
            ops.adamw_flat_lr(st["p"], st["g"], st["m"], st["v"], st["seg_start"], st["seg_wd"], st["seg_lr"], hyper, sqn, max_norm, gs)
        return
    from mtp_amd import _lib
    name = "mtp_adamw_weight_images" if plain else "mtp_adamw_weight_images_lr"
    lrs = [] if plain else [st["seg_lr"].data_ptr()]
    act = _lib.MTP_F32 if KINDS[kind][1] == F32 else _lib.MTP_BF16
    rc = getattr(ops.lib(), name)(st["table"].data_ptr(), *lrs, st["nseg"], st["tiles"], act, st["p"].data_ptr(), st["g"].data_ptr(), st["m"].data_ptr(),
                                  st["v"].data_ptr(), hyper.data_ptr(), None if sqn is None else sqn.data_ptr(), max_norm, gs,
                                  torch.cuda.current_stream().cuda_stream)
    ops.check(rc, name)


def _check_step(what, before, after, ref, cmp):
    """m, v under the counted bounds, p under the measured one, on the elements `cmp`; returns the run's worst p ratio"""
    tiny = 2.0 ** -149
    within(after[1][cmp], ref["m"][cmp], M_K * U * ref["m_terms"][cmp] + tiny, what + " m")
    within(after[2][cmp], ref["v"][cmp], V_K * U * ref["v_terms"][cmp] + tiny, what + " v")
    scale = U * (before[0].double().abs() + ref["update"].abs())[cmp]
    err = (after[0].double() - ref["p"]).abs()[cmp]
    ratio = float((err / scale.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    within(after[0][cmp], ref["p"][cmp], P_K * scale, what + " p")
    return ratio


def _run(ops, kind, form, regime, layout="seam"):
    """the regime's steps of one entry point over one layout, each step checked against adamw_ref from the state it started from, the padding and (fused forms)
    the images checked after each; returns the states as CPU tensors.  Cached: a later test reads the result."""
    key = (kind, form, regime, layout)
    if key in _DONE:
        return _DONE[key]
    rg, plain = REGIMES[regime], form == "plain"
    family, act = KINDS[kind]
    fused = family == "images"
    segs, total = R.layout(LAYOUTS[layout])
    wd, sc = _seg_params(len(segs), rg.get("lr_zero"))
    used, matpad = torch.zeros(total, dtype=torch.bool), torch.zeros(total, dtype=torch.bool)
    for s in segs:
        used[s["off"]:s["off"] + s["numel"]] = True
        if fused and len(s["shape"]) == 2:          # the fused forms never touch the padding behind a matrix; 1-D parameters are rows of 64 WITH their padding
            matpad[s["off"] + s["numel"]:s["off"] + s["padded"]] = True
    cmp = ~matpad
    gen = torch.Generator().manual_seed(17)
    p0 = torch.randn(total, generator=gen) * used
    m0, v0 = torch.zeros(total), torch.zeros(total)
    p0[matpad], m0[matpad], v0[matpad] = 1.5, -0.25, 0.75           # finite sentinels where nothing may be written
    st = dict(p=io(p0), m=io(m0), v=io(v0), nseg=len(segs), seg_start=i64([s["off"] for s in segs]), seg_wd=dev(wd), seg_lr=dev(sc))
    images = None
    if fused:
        images = [((e(*s["shape"], dtype=F32 if s["f32_out"] else act) if s["has_w"] else None),
                   (e(*s["shape"][::-1], dtype=F32 if s["f32_out"] else act) if s["has_wt"] else None)) if len(s["shape"]) == 2 else None for s in segs]
        st["table"] = dev(R.table_bytes(R.wimg_descs(segs, st["p"], images, wd)))
        st["tiles"] = R.total_tiles(segs)
    hist, worst = [], 0.0
    for t in range(1, rg.get("steps", 2) + 1):
        if "g" in rg:
            g = (torch.randint(0, 2, (total,), generator=gen).float() * 2 - 1) * rg["g"] * used
        else:
            g = torch.randn(total, generator=gen) * used
        sumsq = float((g.double() ** 2).sum())
        g_dev = g.clone()
        g_dev[matpad] = float("nan")
        st["g"] = dev(g_dev)
        bc = (1.0, 1.0) if rg.get("late") else (1 - B1 ** t, 1 - B2 ** t)
        hyper_cpu = torch.tensor([LR, B1, B2, EPS, bc[0], bc[1]])
        if rg["sqn"] is None:
            sqn_cpu = None
        elif rg["sqn"] == "true":
            sqn_cpu = torch.tensor([sumsq])
        else:
            sqn_cpu = torch.tensor([(rg["max_norm"] * (1 + rg["sqn"] * 2.0 ** -10) / rg["gs"]) ** 2])
        before = tuple(st[k].cpu() for k in "pmv")
        _adamw_launch(ops, kind, plain, st, dev(hyper_cpu), None if sqn_cpu is None else dev(sqn_cpu), rg["max_norm"], rg["gs"])
        after = tuple(st[k].cpu() for k in "pmv")
        ref = R.adamw_parts(before[0], g, before[1], before[2], [s["off"] for s in segs], wd, None if plain else sc, hyper_cpu, sqn_cpu, rg["max_norm"], rg["gs"])
        what = "%s %s %s %s step %d" % (kind, form, regime, layout, t)
        worst = max(worst, _check_step(what, before, after, ref, cmp))
        for b, a, name in zip(before, after, "pmv"):
            assert torch.equal(bits(a[matpad]), bits(b[matpad])), what + ": the padding behind a matrix was written in " + name
            assert float(a[~used & cmp].abs().sum()) == 0.0, what + ": the zero padding did not stay zero in " + name
        if fused:
            pg = st["p"]
            for s, im in zip(segs, images):
                if im is not None:
                    pv = pg[s["off"]:s["off"] + s["numel"]].view(s["shape"])
                    assert im[0] is None or torch.equal(im[0], pv.to(im[0].dtype)), (what, s["shape"], "w")
                    assert im[1] is None or torch.equal(im[1], pv.t().contiguous().to(im[1].dtype)), (what, s["shape"], "wt")
        hist.append((before, after, ref["gs"]))
    record_parity("step_edges", "adamw_p_ratio %s %s %s %s" % (kind, form, regime, layout), worst)
    out = _DONE[key] = dict(hist=hist, segs=segs, cmp=cmp, used=used, wd=wd, sc=sc, worst=worst)
    return out


@pytest.mark.parametrize("kind,form,regime", CASES)
def test_adamw_matches_the_float64_reference_in_every_regime(ops, kind, form, regime):
    """the seam layout (optim_ref.SEAM_SHAPES, 23 segments with their own weight decay and lr scale) through mtp_adamw_flat[_lr] and mtp_adamw_weight_images[_lr]
    (bf16 and f32 images); per regime what only that regime shows"""
    r = _run(ops, kind, form, regime)
    rg, segs = REGIMES[regime], r["segs"]
    scales = [h[2] for h in r["hist"]]
    if regime in ("clip", "gs8_clip", "lr_zero", "edge_above"):
        assert all(s < rg["gs"] for s in scales)                                # clipping acted
    if regime in ("edge_below", "gs8_noclip", "no_norm"):
        assert all(s == rg["gs"] for s in scales)                               # ... and here it did not
    if regime == "zero_grad":
        (p0, _, _), (p1, m1, v1), _ = r["hist"][0]
        lr = torch.tensor(LR) * (r["sc"] if form == "lr" else torch.ones_like(r["sc"]))
        decay = torch.tensor(1.0) - lr * r["wd"]                                # f32, as the kernel forms it
        assert decay.dtype == F32
        for i, s in enumerate(segs):
            sl = slice(s["off"], s["off"] + s["numel"])
            assert torch.equal(bits(p1[sl]), bits(p0[sl] * decay[i])), s["shape"]
            assert float(r["wd"][i]) != 0.0 or torch.equal(bits(p1[sl]), bits(p0[sl]))
        assert float(m1[r["cmp"]].abs().max()) == 0.0 and float(v1[r["cmp"]].abs().max()) == 0.0
        assert any(float(w) == 0.0 for w in r["wd"])
    if regime == "late_tiny":
        _, (_, _, v1), _ = r["hist"][0]
        assert float(v1[r["used"]].sqrt().max()) < 1e-4 * EPS                   # eps is the denominator
    if regime == "lr_zero":
        for before, after, _ in r["hist"]:
            for j in (LR_ZERO_SEG - 1, LR_ZERO_SEG, LR_ZERO_SEG + 1):
                s = segs[j]
                sl = slice(s["off"], s["off"] + s["numel"])
                same = bits(after[0][sl]) == bits(before[0][sl])
                if j == LR_ZERO_SEG:
                    assert bool(same.all()), "lr scale 0: p moved"
                    assert bool((after[1][sl] != before[1][sl]).all()) and bool((after[2][sl] != before[2][sl]).all())      # ... while m and v did
                else:
                    assert not bool(same.any()), "the neighbour of the lr-scale-0 segment did not update"


@pytest.mark.parametrize("kind,form,regime", [c for c in CASES if c[0] != "flat"])
def test_fused_adamw_leaves_the_state_of_the_flat_one_bit_for_bit(ops, kind, form, regime):
    """test_hip_layer_decay's bit-for-bit property, in every regime: p, m and v of the fused form equal the flat form's from the same state (everywhere but in
    the padding behind matrices, which only the flat form updates)"""
    a, b = _run(ops, kind, form, regime), _run(ops, "flat", form, regime)
    cmp = a["cmp"]
    for (_, fa, _), (_, fb, _) in zip(a["hist"], b["hist"]):
        for x, y, name in zip(fa, fb, "pmv"):
            assert torch.equal(bits(x[cmp]), bits(y[cmp])), name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_adamw_with_a_single_descriptor_or_segment(ops, kind, form):
    """a table of one descriptor, (72, 68) with both images in f32 (ragged in both directions, one quad in the last column group); nseg = 1 for the flat form"""
    r = _run(ops, kind, form, "clip", layout="single")
    assert len(r["segs"]) == 1
    if kind != "flat":
        f = _run(ops, "flat", form, "clip", layout="single")
        assert all(torch.equal(bits(x[r["cmp"]]), bits(y[r["cmp"]])) for (_, fa, _), (_, fb, _) in zip(r["hist"], f["hist"]) for x, y in zip(fa, fb))


@pytest.mark.parametrize("form", FORMS)
def test_adamw_flat_beyond_its_grid(ops, form):
    """8192 workgroups x 256 float4 and 64 elements more: the kernel's stride loop runs; segments of 4 elements at the very start and the very end"""
    n = 4 * 256 * 8192 + 64
    gen = torch.Generator().manual_seed(23)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = 0.1 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen)
    start, wd, sc = [0, 4, n - 4], torch.tensor([0.05, 0.0, 0.1]), torch.tensor([1.0, 0.5, 0.25])
    hyper, sqn = torch.tensor([LR, B1, B2, EPS, 1 - B1 ** 3, 1 - B2 ** 3]), torch.tensor([float((g.double() ** 2).sum())])
    st = dict(p=io(p), g=dev(g), m=io(m), v=io(v), seg_start=i64(start), seg_wd=dev(wd), seg_lr=dev(sc))
    _adamw_launch(ops, "flat", form == "plain", st, dev(hyper), dev(sqn), 5.0, 1.0)
    after = tuple(st[k].cpu() for k in "pmv")
    ref = R.adamw_parts(p, g, m, v, start, wd, sc if form == "lr" else None, hyper, sqn, 5.0, 1.0)
    assert ref["gs"] < 1.0
    worst = _check_step("flat %s beyond the grid" % form, (p, m, v), after, ref, torch.ones(n, dtype=torch.bool))
    record_parity("step_edges", "adamw_p_ratio flat %s clip large" % form, worst)


@pytest.mark.parametrize("act", DT, ids=["f32", "bf16"])
def test_weight_images_over_the_seam_shapes(ops, act):
    """mtp_weight_images through ops.WeightImages: every matrix of the seam layout, its images NaN-poisoned; again after the masters changed in place"""
    mats = [s for s in R.SEAM_SHAPES if len(s[0]) == 2]
    srcs = [io(rnd(*s[0], seed=i)) for i, s in enumerate(mats)]
    entries = []
    for src, (shape, has_w, has_wt, f32_out) in zip(srcs, mats):
        dt = F32 if f32_out else act
        entries.append((src, e(*shape, dtype=dt) if has_w else None, e(*shape[::-1], dtype=dt) if has_wt else None, f32_out))
    wi = ops.WeightImages(entries, act)
    for rep in range(2):
        snap = [s.clone() for s in srcs]
        wi.refresh()
        for src, was, (_, w, wt, _), (shape, _, _, _) in zip(srcs, snap, entries, mats):
            assert torch.equal(bits(src), bits(was))                               # the master is an input
            assert w is None or torch.equal(w, src.to(w.dtype)), (shape, rep, "w")
            assert wt is None or torch.equal(wt, src.t().contiguous().to(wt.dtype)), (shape, rep, "wt")
        for s in srcs:
            s.mul_(-1.7).add_(0.3)


# ------------------------------------------------------------------------------------------------ glue
COPY_COUNTS = [1, 3, 255, 256, 257, 65535, 65536, 65537, 131073, 1, 4, 64]


def test_copy_segments_up_to_and_past_its_grid(ops):
    """twelve copies in one launch; the grid is sized for 65536 floats per segment, so 65537 and 131073 run the stride loop"""
    srcs = [rnd(n, seed=30 + i) for i, n in enumerate(COPY_COUNTS)]
    dsts = [e(n) for n in COPY_COUNTS]
    ops.copy_segments([dev(s) for s in srcs], dsts)
    for s, d in zip(srcs, dsts):
        assert torch.equal(d.cpu(), s)


def test_copy_segments_refuses_thirteen_segments_and_an_empty_one(ops):
    src, dst = dev(rnd(64)), ARENA.wide(1, 64)           # no column registered: all of dst must stay poison
    P13, P2 = C.c_void_p * 13, C.c_void_p * 2
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_copy_segments_f32"):
        ops.check(ops.lib().mtp_copy_segments_f32(P13(*[src.data_ptr()] * 13), P13(*[dst.data_ptr()] * 13), (C.c_int64 * 13)(*[4] * 13), 13, st), "mtp_copy_segments_f32")
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_copy_segments_f32"):
        ops.check(ops.lib().mtp_copy_segments_f32(P2(*[src.data_ptr()] * 2), P2(*[dst.data_ptr()] * 2), (C.c_int64 * 2)(4, 0), 2, st), "mtp_copy_segments_f32")
    torch.cuda.synchronize()
    ARENA.check()


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("Hp,Wp", [(1, 1), (1, 2), (3, 5)])
@pytest.mark.parametrize("Cin", [1, 3])
@pytest.mark.parametrize("P", [4, 16])
def test_patchify_unpatchify_edge_grids(ops, dtype, Hp, Wp, Cin, P):
    """whole grids of 1, 2 and 15 patches, then an image with rows (and, where W % 4 == 0 allows it, columns) beyond the last whole patch: patchify ignores them,
    unpatchify leaves them exactly 0 (its memset branch) and nothing poisoned"""
    B, K = 2, Cin * P * P
    img = rnd(B, Cin, Hp * P, Wp * P, dtype=dtype)
    cols = ops.patchify(dev(img), e(B * Hp * Wp, K, dtype=dtype), P)
    ref, grid = O.patchify(img, P)
    assert grid == (Hp, Wp) and torch.equal(cols.float().cpu(), ref)
    assert torch.equal(ops.unpatchify(ARENA.frozen(cols), e(B, Cin, Hp * P, Wp * P), P).cpu(), img)
    H, W = Hp * P + P - 1, Wp * P + (4 if P > 4 else 0)
    assert H % P and W % 4 == 0 and (P == 4 or W % P)
    img2 = rnd(B, Cin, H, W, dtype=dtype, seed=1)
    cols2 = ops.patchify(dev(img2), e(B * Hp * Wp, K, dtype=dtype), P)
    ref2, _ = O.patchify(img2, P)
    assert torch.equal(cols2.float().cpu(), ref2)
    back = ops.unpatchify(ARENA.frozen(cols2), e(B, Cin, H, W), P).cpu()
    want = torch.zeros(B, Cin, H, W)
    want[:, :, :Hp * P, :Wp * P] = img2[:, :, :Hp * P, :Wp * P]
    assert torch.equal(bits(back), bits(want)) and torch.equal(back, O.unpatchify(ref2, B, Cin, H, W, P))


@pytest.mark.parametrize("H,W,P", [(8, 16, 16), (16, 18, 16), (12, 12, 6)], ids=["H<P", "W%4", "P%4"])
def test_patchify_unpatchify_refuse_without_writing(ops, H, W, P):
    img, cols = dev(rnd(1, 1, H, W)), dev(rnd(1, P * P))
    out = ARENA.wide(1, max(H * W, P * P))               # no column registered: all of it must stay poison
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_patchify"):
        ops.patchify(img, out[:, :P * P], P)
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_unpatchify"):
        ops.unpatchify(cols, out[:, :H * W].view(1, 1, H, W), P)
    torch.cuda.synchronize()
    ARENA.check()


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (32, 32), (33, 4), (31, 36)])
def test_preprocess_patchify_edge_images(ops, dtype, H, W, flip):
    """one pixel, a few, exactly one padded block, one row past it; W off 4 (byte loads) and on 4 (dword loads, (33, 4) and (31, 36) with padding beside them)"""
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    img = torch.randint(0, 256, (2, H, W, 3), generator=torch.Generator().manual_seed(H * 100 + W), dtype=torch.uint8)
    ref, (Hp, Wp) = O.patchify(O.preprocess(img, mean, std, bgr_to_rgb=flip, pad_size_divisor=32, pad_value=-1.5))
    assert (Hp, Wp) == ops.padded_grid(H, W, 16, 32)
    cols = ops.preprocess_patchify(dev(img), e(2 * Hp * Wp, 768, dtype=dtype), 16, mean, std, bgr_to_rgb=flip, pad_divisor=32, pad_value=-1.5)
    assert torch.equal(cols.cpu(), ref.to(dtype))


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cin,Cout", [(8, 8), (8, 72), (72, 8), (64, 64), (1, 1), (1, 9), (7, 8), (12, 20)])
def test_convt_pack_and_unpack_edge_channels(ops, dtype, Cin, Cout):
    """the tiled kernels from their smallest channel counts (8) to one whole tile, the element-wise ones from one channel; each image alone and both"""
    cw = rnd(Cin, Cout, 2, 2, seed=3)
    ref = O.convT_gemm_weight(cw)
    dcw = dev(cw)
    for want_g, want_t in ((True, False), (False, True), (True, True)):
        wg, wgT = (e(4 * Cout, Cin, dtype=dtype) if want_g else None), (e(Cin, 4 * Cout, dtype=dtype) if want_t else None)
        ops.convt_pack(dcw, wg, wgT)
        assert wg is None or torch.equal(wg.cpu(), ref.to(dtype)), (want_g, want_t)
        assert wgT is None or torch.equal(wgT.cpu(), ref.t().contiguous().to(dtype)), (want_g, want_t)
    dwg = rnd(4 * Cout, Cin, seed=4)
    dw = ops.convt_unpack_grad(dev(dwg), e(Cin, Cout, 2, 2))
    wr = cw.clone().requires_grad_(True)
    (O.convT_gemm_weight(wr) * dwg).sum().backward()
    assert torch.equal(dw.cpu(), wr.grad)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 2, 255, 257])
@pytest.mark.parametrize("Cc", [4, 12, 260])
def test_colsum_returns_the_integers(ops, dtype, rows, Cc):
    """the narrowest width, a ragged one and one past the 256 columns of a workgroup; plain into a poisoned output, accumulating on top of integers"""
    x = R.exact_ints(rows * Cc, seed=3).view(rows, Cc)
    dx, want = dev(x, dtype), x.double().sum(0)
    assert torch.equal(ops.colsum(dx, e(Cc)).cpu().double(), want)
    base = (torch.arange(Cc) % 7 - 3).float()
    acc = ops.colsum(dx, io(base), accumulate=True)
    assert torch.equal(acc.cpu().double(), base.double() + want)
    ops.colsum(dx, acc, accumulate=True)
    assert torch.equal(acc.cpu().double(), base.double() + 2 * want)


@pytest.mark.parametrize("rows", [1, 2, 255, 257])
@pytest.mark.parametrize("Rr,Cc,extra", [(1, 1, 0), (3, 5, 0), (16, 4, 0), (3, 5, 1)])
def test_reduce_rows_transposed_returns_the_integers(ops, rows, Rr, Cc, extra):
    """mtp_reduce_rows_t_f32 (no wrapper: through _lib) and its batched form (ops.reduce_rows_deferred): column a C + b of the partial rows -> out[b R + a];
    extra: a row stride wider than R C"""
    ld = Rr * Cc + extra
    x = R.exact_ints(rows * ld, seed=4).view(rows, ld)
    want = x[:, :Rr * Cc].double().sum(0).view(Rr, Cc).t().reshape(-1)
    dx, st = dev(x), torch.cuda.current_stream().cuda_stream
    out = e(Rr * Cc)
    ops.check(ops.lib().mtp_reduce_rows_t_f32(dx.data_ptr(), ld, out.data_ptr(), rows, Rr, Cc, 0, st), "mtp_reduce_rows_t_f32")
    assert torch.equal(out.cpu().double(), want)
    base = (torch.arange(Rr * Cc) % 5 - 2).float()
    acc = io(base)
    ops.check(ops.lib().mtp_reduce_rows_t_f32(dx.data_ptr(), ld, acc.data_ptr(), rows, Rr, Cc, 1, st), "mtp_reduce_rows_t_f32")
    assert torch.equal(acc.cpu().double(), base.double() + want)
    part = dx[:, :Rr * Cc]
    o1, o2 = e(Rr * Cc), io(base)
    ops.reduce_rows_deferred([(part, o1, False, (Rr, Cc))])
    ops.reduce_rows_deferred([(part, o2, True, (Rr, Cc)), (part, acc, True, (Rr, Cc))])
    assert torch.equal(o1.cpu().double(), want) and torch.equal(o2.cpu().double(), base.double() + want)
    assert torch.equal(acc.cpu().double(), base.double() + 2 * want)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("njobs", [1, 12, 13])
def test_sum_partials_batches_of_one_twelve_and_thirteen(ops, dtype, njobs):
    """split-K partial tiles of the smallest TN problems, left in (poisoned) workspaces and summed later, twelve GEMMs per launch: bit-equal to the immediate path"""
    E = 8 if dtype == BF16 else 4
    shapes = [(65, 17, 16, 2), (200, 1, 33, 3), (130, 16, 17, 2)]
    jobs, outs, refs = [], [], []
    for i in range(njobs):
        Kc, Mq, Nq, split = shapes[i % 3]
        a, b = dev(rnd(Kc, Mq * E, dtype=dtype, scale=0.5, seed=i), dtype), dev(rnd(Kc, Nq * E, dtype=dtype, seed=50 + i, scale=0.5), dtype)
        refs.append(ops.gemm_tn(a, b, e(Mq * E, Nq * E), split_k=split))
        outs.append(ops.gemm_tn(a, b, e(Mq * E, Nq * E), split_k=split, defer=jobs))
    assert len(jobs) == njobs and all(j[3] > 1 for j in jobs)
    ops.sum_partials(jobs)
    assert not jobs
    for o, r in zip(outs, refs):
        assert torch.equal(bits(o), bits(r)) and not bool(o.isnan().any())
