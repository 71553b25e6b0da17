"""GPU: the smallest and the most ragged shapes the C ABI accepts, every buffer out of the guard arena (tests/guard.py): outputs NaN-poisoned and
between guards, inputs frozen, the wrappers' workspaces poisoned and guarded.  References are the same operation in float64 on the CPU, computed
from the dtype-rounded inputs.

The plain / bias / residual NT epilogues and the TN GEMM are held to an element-wise bound that follows from the arithmetic, not from a measurement:
exact products (bf16 x bf16 fits f32; f32 x f32 rounds once) accumulated in f32 over K terms, then the epilogue adds, then one rounding of the output:

    |got - ref| <= 2 K 2^-24 (|a| |w|^T + |bias| + |res|)  [+ 2^-8 |ref| for a bf16 output]

(the factor 2 covers the epilogue adds and the order of accumulation; the row scales used here are <= 1, so scaling only shrinks the error).
GELU / GELU' / MUL epilogues and the row-wise ops use the project's TOL table (max error relative to the tensor's max)."""
import pytest
import torch
import torch.nn.functional as F

import guard
from conftest import rel_err
from mtp_amd._lib import GEMM_NT_P8, GEMM_NT_P8_224, GEMM_NT_P8_256, GEMM_NT_REG_STAGED, GEMM_NT_SB8, GEMM_NT_STRIP
from oracle import vit_rvsa_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
TOL = {F32: 2e-4, BF16: 1.5e-2}
ARENA = None     # the running test's guard.Arena
# what _lib.check raises for MTP_ERR_ARG (-1) and for nothing else: an unsupported configuration (-2) and a launch that was tried and failed
# (a hipError_t) carry other texts, so a refusal test that matches this saw the argument check itself
ERR_ARG = r"^%s failed: invalid argument$"


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


def gemm_bound(K, mag, ref, out_dtype):
    b = 2.0 * K * 2.0 ** -24 * mag.double()
    return b + 2.0 ** -8 * ref.double().abs() if out_dtype == BF16 else b


# ------------------------------------------------------------------------------------------------ gemm_nt
FAMILIES = [0, GEMM_NT_REG_STAGED, GEMM_NT_SB8]                         # the 128-wide kernels: default (LDS-DMA on whole K tiles) / register-staged / 256 x 128 8-wave
FALL_THROUGH = [GEMM_NT_P8, GEMM_NT_P8_224, GEMM_NT_P8_256, GEMM_NT_STRIP]            # pipelined (auto, 224, 256 rows) / strip: take none of the ragged shapes below
MS, NS = [1, 7, 127, 129, 255, 257], [4, 12, 132, 260]
KS = {BF16: [8, 72, 200, 64], F32: [4, 36, 100, 32]}       # ragged K (register-staged loads) and one whole K tile (64 bf16 / 32 f32: the LDS-DMA kernels)
EPIS = ["none", "bias", "res_rowscale", "res_mod", "bias_mod", "gelu_aux", "gelu_dg", "mul", "n_slice"]
BIAS_MOD = {4: 4, 12: 4, 132: 44, 260: 52, 8: 4, 24: 12, 136: 68, 264: 132}


def _nt_cases(count=18):
    """thinned cross product: `count` cases per (dtype, variant); from 9 on, every M, N, K and epilogue appears with every variant"""
    out = []
    for j in range(count):
        out.append((j % 6, (j + j // 4) % 4, (j + j // 6) % 4, EPIS[j % 9]))
    assert {c[0] for c in out} == set(range(6)) and {c[1] for c in out} == set(range(4)) and {c[2] for c in out} == set(range(4)) and {c[3] for c in out} == set(EPIS)
    return out


def _run_nt(ops, dtype, variant, M, N, K, epi, want_tile):
    a, w = rnd(M, K, dtype=dtype), rnd(N, K, dtype=dtype, seed=1, scale=0.5)
    b = rnd(N, seed=2)
    da, dw, db = dev(a, dtype), dev(w, dtype), dev(b)
    prod, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    kw, out_dtype, bound_ok = dict(variant=variant), dtype, True
    if epi == "none":
        ref = prod
    elif epi == "bias":
        kw.update(bias=db)
        ref, mag = prod + b.double(), mag + b.double().abs()
    elif epi == "res_rowscale":
        rps = 1 if M == 1 else 3
        rs = torch.tensor([0.0, 1.0, 0.5])[torch.arange((M + rps - 1) // rps) % 3]
        res = rnd(M, N, seed=3)
        kw.update(epi=ops.EPI_BIAS_RES, bias=db, res=dev(res), rowscale=dev(rs), rows_per_sample=rps)
        out_dtype = F32
        ref = res.double() + rs.double().repeat_interleave(rps)[:M, None] * (prod + b.double())
        mag = mag + b.double().abs() + res.double().abs()
    elif epi == "res_mod":
        rm = min(M, 5)
        pos = rnd(rm, N, seed=4)
        kw.update(epi=ops.EPI_BIAS_RES, bias=db, res=dev(pos), res_mod=rm)
        out_dtype = F32
        full = pos.double()[torch.arange(M) % rm]
        ref, mag = full + prod + b.double(), mag + b.double().abs() + full.abs()
    elif epi == "bias_mod":
        bm = BIAS_MOD[N]
        b4 = rnd(bm, seed=6)
        kw.update(bias=dev(b4), bias_mod=bm)
        out_dtype = F32                                   # f32 out from ACT in (ConvTranspose2d's repeated bias)
        rep = b4.double().repeat(N // bm)
        ref, mag = prod + rep, mag + rep.abs()
    elif epi in ("gelu_aux", "gelu_dg"):
        bound_ok = False
        ref = prod + b.double()
    elif epi == "mul":
        bound_ok = False
        fac = rnd(M, N, dtype=dtype, seed=7)
        kw.update(epi=ops.EPI_MUL, aux=dev(fac, dtype))
        ref = prod * fac.double()
    elif epi == "n_slice":
        kw.update(bias=db)
        ref, mag = prod + b.double(), mag + b.double().abs()
    if epi == "n_slice":
        # the first N columns of a wider out; w holds more rows than are used.  The other columns must keep their poison (checked like guards).
        wide = ARENA.wide(M, N + 12, dtype=out_dtype)
        ARENA.cols(wide, 0, N)
        w_more = torch.cat([w, rnd(8, K, dtype=dtype, seed=9)])
        dwm = dev(w_more, dtype)
        assert ops.gemm_nt_tile(da, dwm, wide, n=N, **kw) == want_tile
        ops.gemm_nt(da, dwm, wide, n=N, **kw)
        got = wide[:, :N]
    else:
        out = e(M, N, dtype=out_dtype)
        if epi == "gelu_aux":
            aux = e(M, N, dtype=dtype)
            kw.update(epi=ops.EPI_BIAS_GELU, bias=db, aux=aux)
        elif epi == "gelu_dg":
            aux = e(M, N, dtype=dtype)
            kw.update(epi=ops.EPI_BIAS_GELU_DG, bias=db, aux=aux)
        assert ops.gemm_nt_tile(da, dw, out, **kw) == want_tile       # the family that really runs: asserted, not assumed
        got = ops.gemm_nt(da, dw, out, **kw)
    what = "gemm_nt %s M=%d N=%d K=%d %s variant=%d" % (str(dtype)[6:], M, N, K, epi, variant)
    if bound_ok:
        within(got, ref, gemm_bound(K, mag, ref, out_dtype), what)
    elif epi == "gelu_aux":
        assert rel_err(aux.float().cpu(), ref) < TOL[dtype] and rel_err(got.float().cpu(), O.gelu(ref.float())) < TOL[dtype], what
    elif epi == "gelu_dg":
        assert rel_err(got.float().cpu(), O.gelu(ref.float())) < TOL[dtype] and rel_err(aux.float().cpu(), O.dgelu(ref.float())) < TOL[dtype], what
    else:
        assert rel_err(got.float().cpu(), ref) < TOL[dtype], what
    ARENA.check_written(got, what)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("variant", FAMILIES)
@pytest.mark.parametrize("mi,ni,ki,epi", _nt_cases())
def test_gemm_nt_edge_shapes(ops, dtype, variant, mi, ni, ki, epi):
    """M down to 1, N down to 4, a partial tile in both directions, K below and off the K tile, on the 128-wide kernels (LDS-DMA form for K = 64 / 32,
    register-staged otherwise; 256 x 128 tiles with GEMM_NT_SB8)"""
    _run_nt(ops, dtype, variant, MS[mi], NS[ni], KS[dtype][ki], epi, 128)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("variant", FALL_THROUGH)
@pytest.mark.parametrize("mi,ni,ki,epi", _nt_cases(9))
def test_gemm_nt_edge_shapes_fall_through(ops, dtype, variant, mi, ni, ki, epi):
    """with these contractions (K < 128, or off 64) and row / column counts off 8, neither the pipelined (GEMM_NT_P8 / _224 / _256) nor the strip kernel
    (GEMM_NT_STRIP) takes the problem: gemm_nt_tile must say 128, i.e. the forced variant falls through to the default kernel, and the result holds all the same.
    Nine cases each: every M, N, K and epilogue once (the kernel that runs is the one the 18 cases of variant 0 above already sweep)"""
    _run_nt(ops, dtype, variant, MS[mi], NS[ni], KS[dtype][ki], epi, 128)


# the smallest / most ragged problems the pipelined and the strip kernel themselves accept: M, N multiples of 8 from 8 up; K = 128 (one K-tile pair) resp.
# 704 (11 K tiles) -- here gemm_nt_tile must name those families.  All nine epilogues: the pipelined kernel has an instantiation for each; the strip
# kernel has none for GELU + aux and takes no res_mod (mtp_nt_s8_fits) -- those two must fall through to the 128-wide kernels, which is asserted.
P8S8 = [(GEMM_NT_P8, 256, 128), (GEMM_NT_P8_224, 256, 128), (GEMM_NT_P8_256, 256, 256), (GEMM_NT_STRIP, 64, 704)]
P8S8_SHAPES = [(8, 8), (8, 264), (264, 8), (136, 136), (520, 24)]


def _p8s8_cases():
    """per variant 27 of the 45 (shape, epilogue) pairs: every epilogue at three shapes, every shape with five or six epilogues"""
    out = []
    for variant, tile, K in P8S8:
        for j in range(27):
            epi = EPIS[j % 9]
            out.append((variant, 128 if variant == GEMM_NT_STRIP and epi in ("res_mod", "gelu_aux") else tile, K) + P8S8_SHAPES[j % 5] + (epi,))
    return out


@pytest.mark.parametrize("variant,tile,K,M,N,epi", _p8s8_cases())
def test_gemm_nt_pipelined_and_strip_kernels_at_their_smallest_shapes(ops, variant, tile, K, M, N, epi):
    _run_nt(ops, BF16, variant, M, N, K, epi, tile)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
def test_gemm_nt_refuses_illegal_shapes_without_launching(ops, dtype):
    """N % 4, K % E (8 bf16 / 4 f32) and a base pointer off 16 bytes must come back as MTP_ERR_ARG with nothing written: every output stays poison"""
    E = 8 if dtype == BF16 else 4
    M, N, K = 16, 16, 4 * E

    def refused(a, w, out, **kw):
        with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_gemm_nt"):
            ops.gemm_nt(a, w, out, **kw)
        torch.cuda.synchronize()
    a, w = dev(rnd(M, K, dtype=dtype), dtype), dev(rnd(N, K, dtype=dtype, seed=1), dtype)
    wide = ARENA.wide(M, N, dtype=dtype)                                  # no column registered: the whole buffer must stay poison
    refused(a, w, wide, n=N - 2)                                          # N % 4 != 0
    refused(a, w, wide, n=N - 1)
    for Kb in (K + E // 2, K + 1) if dtype == BF16 else (K + 2, K + 1):   # K % E != 0 (lda / ldb with it)
        refused(dev(rnd(M, Kb, dtype=dtype), dtype), dev(rnd(N, Kb, dtype=dtype, seed=1), dtype), wide)
    # pointers off 16 bytes: views that start one element (bf16: 2 bytes, f32: 4 bytes) into a buffer
    big_a, big_w, big_o = dev(rnd(M * K + E, dtype=dtype), dtype), dev(rnd(N * K + E, dtype=dtype, seed=1), dtype), ARENA.wide(1, M * N + 8, dtype=dtype)
    a1, w1, o1 = big_a[1:1 + M * K].view(M, K), big_w[1:1 + N * K].view(N, K), big_o[0, 1:1 + M * N].view(M, N)
    assert a1.data_ptr() % 16 and w1.data_ptr() % 16 and o1.data_ptr() % 16
    refused(a1, w, wide)
    refused(a, w1, wide)
    refused(a, w, o1)
    ARENA.check()


# ------------------------------------------------------------------------------------------------ gemm_tn
@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("with_cs", [False, True])
@pytest.mark.parametrize("Kc,Mq,Nq,split", [(1, 1, 1, 1), (3, 1, 17, 1), (64, 16, 1, 1), (65, 17, 16, 2), (200, 1, 33, 3), (129, 33, 1, None), (64, 16, 16, 1), (130, 16, 17, 2)])
def test_gemm_tn_edge_shapes(ops, dtype, with_cs, Kc, Mq, Nq, split):
    """the ungrouped kernel: M and N in units of E (8 bf16 / 4 f32 -- the smallest the ABI takes), one element / one tile / just past a 128 tile,
    contractions of one row, off the K tile and split"""
    E = 8 if dtype == BF16 else 4
    M, N = Mq * E, Nq * E
    a, b = rnd(Kc, M, dtype=dtype, scale=0.5), rnd(Kc, N, dtype=dtype, seed=1, scale=0.5)
    cs0 = rnd(M, seed=2)
    cs = io(cs0) if with_cs else None
    out = ops.gemm_tn(dev(a, dtype), dev(b, dtype), e(M, N), split_k=split, colsum=cs)
    ref, mag = a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs()
    within(out, ref, gemm_bound(Kc, mag, ref, F32), "gemm_tn K=%d M=%d N=%d split=%s" % (Kc, M, N, split))
    if with_cs:
        assert rel_err(cs.cpu(), cs0.double() + a.double().sum(0)) < 1e-4


@pytest.mark.parametrize("with_cs", [False, True])
@pytest.mark.parametrize("shapes", [[(128, 8, 8)], [(128, 8, 264), (128, 264, 8)], [(256, 256, 256), (128, 264, 264)], [(384, 16, 248), (128, 520, 8), (128, 8, 8)]])
def test_wgrad_queue_smallest_and_just_past_a_tile(ops, with_cs, shapes):
    """the grouped kernel at the smallest problem WgradQueue.add queues (K = 128, M = N = 8) and one 8-column step past the 256 tile"""
    q, keep = ops.WgradQueue(), []
    for i, (Kc, M, N) in enumerate(shapes):
        a, b = rnd(Kc, M, dtype=BF16, scale=0.5, seed=i), rnd(Kc, N, dtype=BF16, scale=0.5, seed=40 + i)
        cs0 = rnd(M, seed=80 + i)
        cs, dw = (io(cs0) if with_cs else None), e(M, N)
        assert q.add(dev(a, BF16), dev(b, BF16), dw, cs)
        keep.append((a, b, cs0, cs, dw, Kc))
    q.flush()
    for a, b, cs0, cs, dw, Kc in keep:
        ref, mag = a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs()
        within(dw, ref, gemm_bound(Kc, mag, ref, F32), "grouped gemm_tn K=%d %s" % (Kc, tuple(dw.shape)))
        if with_cs:
            assert rel_err(cs.cpu(), cs0.double() + a.double().sum(0)) < 1e-4


def test_gemm_tn_refuses_illegal_shapes_without_launching(ops):
    a, b = dev(rnd(16, 12, dtype=BF16), BF16), dev(rnd(16, 16, dtype=BF16, seed=1), BF16)       # M % 8 != 0
    out = ARENA.wide(12, 16)
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_gemm_tn"):
        ops.gemm_tn(a, b, out)
    torch.cuda.synchronize()
    ARENA.check()


# ------------------------------------------------------------------------------------------------ row-wise ops
ROWS = [1, 2, 63, 65]


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("Cc", [4, 2048])          # the narrowest and the widest row the LayerNorm kernels take
def test_layernorm_edge_rows(ops, dtype, rows, Cc):
    x, g, b = rnd(rows, Cc, scale=2.0) + 0.5, 1 + 0.1 * rnd(Cc, seed=1), 0.1 * rnd(Cc, seed=2)
    mean, rstd = e(rows), e(rows)
    y = ops.layernorm_fwd(dev(x), dev(g), dev(b), e(rows, Cc, dtype=dtype), mean, rstd)
    yr, mr, rr = O.layernorm_fwd(x.double(), g.double(), b.double())
    assert rel_err(y.float().cpu(), yr) < TOL[dtype] and rel_err(mean.cpu(), mr) < 1e-5 and rel_err(rstd.cpu(), rr) < 1e-5
    dy, dres, extra = rnd(rows, Cc, dtype=dtype, seed=3), rnd(rows, Cc, seed=4), rnd(rows, Cc, seed=5)
    rps = rows // 2 if rows % 2 == 0 else rows
    cs = torch.tensor([0.5, 2.0])[: rows // rps]
    dx, dxc, dg, db = e(rows, Cc), e(rows, Cc, dtype=dtype), e(Cc), e(Cc)
    ops.layernorm_bwd(dev(dy, dtype), dev(x), mean, rstd, dev(g), dx, dg, db, dres=dev(dres), extra=dev(extra), dx_copy=dxc, copy_scale=dev(cs), rows_per_sample=rps)
    dxr, dgr, dbr = O.layernorm_bwd(dy.double(), x.double(), mr, rr, g.double())
    tot = dxr + dres.double() + extra.double()
    assert rel_err(dx.cpu(), tot) < 2e-4 and rel_err(dxc.float().cpu(), tot * cs.double().repeat_interleave(rps)[:, None]) < TOL[dtype]
    assert rel_err(dg.cpu(), dgr) < 2e-4 and rel_err(db.cpu(), dbr) < 2e-4
    dg2, db2, dx2 = io(torch.ones(Cc)), io(torch.full((Cc,), -2.0)), e(rows, Cc)
    ops.layernorm_bwd(dev(dy, dtype), dev(x), mean, rstd, dev(g), dx2, dg2, db2, accumulate=True)
    assert rel_err(dg2.cpu(), 1 + dgr) < 2e-4 and rel_err(db2.cpu(), dbr - 2) < 2e-4 and rel_err(dx2.cpu(), dxr) < 2e-4


@pytest.mark.parametrize("Hp,Wp,B", [(1, 1, 1), (7, 9, 1), (8, 8, 2)])
def test_layernorm_bwd_window_addend_edge_grids(ops, Hp, Wp, B):
    """win_add on a one-token grid (one window of which 48 positions are padding), on 7 x 9 -> 7 x 14 (two windows) and on two images of 8 x 8 -> 14 x 14 (four each)"""
    Cc = 4
    T = B * Hp * Wp
    nh, nw = ops.rvsa_windows(Hp, Wp)
    pt, pl = ((7 - Hp % 7) % 7) // 2, ((7 - Wp % 7) % 7) // 2
    x, dy, gamma = rnd(T, Cc, scale=2.0) + 0.5, rnd(T, Cc, seed=1), 1.0 + 0.1 * rnd(Cc, seed=2)
    add = rnd(B * nh * nw, Cc, seed=3)
    win = (((torch.arange(Hp) + pt) // 7)[:, None] * nw + ((torch.arange(Wp) + pl) // 7)[None, :]).reshape(-1)
    win_all = (torch.arange(B)[:, None] * (nh * nw) + win[None, :]).reshape(-1)
    _, mr, rr = O.layernorm_fwd(x.double(), gamma.double(), torch.zeros(Cc).double())
    dxr, dgr, dbr = O.layernorm_bwd(dy.double() + add.double()[win_all], x.double(), mr, rr, gamma.double())
    dx, dg, db = e(T, Cc), e(Cc), e(Cc)
    ops.layernorm_bwd(dev(dy), dev(x), dev(mr.float()), dev(rr.float()), dev(gamma), dx, dg, db, win_add=dev(add), grid=(B, Hp, Wp))
    assert rel_err(dx.cpu(), dxr) < 2e-4 and rel_err(dg.cpu(), dgr) < 2e-4 and rel_err(db.cpu(), dbr) < 2e-4


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("Cc", [4, 2048])
def test_layernorm_residual_edge_rows(ops, dtype, rows, Cc):
    rps = 2
    ns = (rows + rps - 1) // rps
    h, x, dout = rnd(rows, Cc, dtype=dtype, seed=1), rnd(rows, Cc, seed=2), rnd(rows, Cc, seed=3)
    g, b, ls = 1.0 + 0.1 * rnd(Cc, seed=4), 0.1 * rnd(Cc, seed=5), 0.5 * rnd(Cc, seed=6)
    ss = (torch.arange(ns) % 3 != 1).float() / 0.8
    hr, gr, br, lr = (t.double().clone().requires_grad_(True) for t in (h, g, b, ls))
    ref = x.double() + ss.double().repeat_interleave(rps)[:rows, None] * lr * F.layer_norm(hr, (Cc,), gr, br, 1e-6)
    ref.backward(dout.double())
    out, oact, mean, rstd = e(rows, Cc), e(rows, Cc, dtype=dtype), e(rows), e(rows)
    ops.layernorm_residual_fwd(dev(h, dtype), dev(g), dev(b), dev(x), dev(ls), out, oact, mean, rstd, dev(ss), rps)
    assert rel_err(out.cpu(), ref.detach()) < 1e-5 and rel_err(oact.float().cpu(), ref.detach()) < (1e-5 if dtype == F32 else 1e-2)
    dh, dg, db, dl = e(rows, Cc, dtype=dtype), ARENA.zeros(Cc), ARENA.zeros(Cc), ARENA.zeros(Cc)      # (the three parameter gradients accumulate)
    ops.layernorm_residual_bwd(dev(dout), dev(h, dtype), mean, rstd, dev(g), dev(b), dev(ls), dh, dg, db, dl, dev(ss), rps)
    assert rel_err(dh.float().cpu(), hr.grad) < (1e-4 if dtype == F32 else 1e-2)
    assert rel_err(dg.cpu(), gr.grad) < 1e-4 and rel_err(db.cpu(), br.grad) < 1e-4 and rel_err(dl.cpu(), lr.grad) < 1e-4


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("Cc", [4, 2052])
def test_reductions_casts_axpy_edge_rows(ops, dtype, rows, Cc):
    dy = rnd(rows, Cc, dtype=dtype)
    assert rel_err(ops.colsum(dev(dy, dtype), e(Cc)).cpu(), dy.double().sum(0)) < 2e-4
    g0 = rnd(Cc, seed=3)
    assert rel_err(ops.colsum(dev(dy, dtype), io(g0), accumulate=True).cpu(), g0.double() + dy.double().sum(0)) < 2e-4
    part = rnd(rows, Cc + 8, seed=4)
    dpart = dev(part)
    assert rel_err(ops.reduce_rows(dpart, e(Cc + 8)).cpu(), part.double().sum(0)) < 2e-4
    assert rel_err(ops.reduce_rows(dpart[:, 8:], io(g0), accumulate=True).cpu(), g0.double() + part.double()[:, 8:].sum(0)) < 2e-4      # a column slice, accumulating
    src = rnd(rows, Cc, seed=5)
    n1 = rows * Cc - 1                                                  # a count that is not a multiple of 4
    if dtype == BF16:
        assert torch.equal(ops.cast(dev(src), e(rows, Cc, dtype=dtype)).cpu(), src.to(dtype))
    assert torch.equal(ops.cast(dev(src.reshape(-1)[:n1]), e(n1, dtype=BF16)).cpu(), src.reshape(-1)[:n1].to(BF16))
    assert torch.equal(ops.cast(dev(src.reshape(-1)[:n1].to(BF16)), e(n1)).cpu(), src.reshape(-1)[:n1].to(BF16).float())
    sc = torch.tensor([2.0, 0.0, 0.5])[torch.arange(rows) % 3]
    out = ops.scale_rows_cast(dev(src), e(rows, Cc, dtype=dtype), dev(sc), 1)
    assert rel_err(out.float().cpu(), src.double() * sc.double()[:, None]) < TOL[dtype]
    assert torch.equal(ops.scale_rows_cast(dev(src), e(rows, Cc, dtype=dtype)).cpu(), src.to(dtype))
    y, x = rnd(n1, seed=6), rnd(n1, seed=7)
    assert rel_err(ops.axpy(io(y), dev(x), 0.5).cpu(), y.double() + 0.5 * x.double()) < 1e-6
    t = ops.transpose_cast(dev(src), e(Cc, rows, dtype=dtype))
    assert torch.equal(t.cpu(), src.t().contiguous().to(dtype))


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,Hp,Wp", [(1, 1, 1), (1, 1, 2), (1, 7, 9), (1, 5, 13), (2, 3, 3)])      # 1, 2, 63, 65 positions per image; two images
@pytest.mark.parametrize("Cc", [4, 68, 1032])          # (channels come in fours: see test_layout_ops_refuse_channels_off_four)
@pytest.mark.parametrize("L", [0, 1])
def test_tokens_nchw_edge_grids(ops, dtype, B, Hp, Wp, Cc, L):
    x = rnd(B * Hp * Wp * 4 ** L, Cc, dtype=dtype)
    f = ops.tokens_to_nchw(dev(x, dtype), e(B, Cc, Hp << L, Wp << L, dtype=dtype), B, Hp, Wp, L)
    assert torch.equal(f.float().cpu(), O.tokens_to_nchw(x, B, Hp, Wp, L))
    back = ops.nchw_to_tokens(ARENA.frozen(f), e(x.shape[0], Cc, dtype=dtype), B, Hp, Wp, L)
    assert torch.equal(back.float().cpu(), x)
    if dtype == BF16:       # f32 tokens -> ACT map and back (what the FPN tail does)
        f5 = ops.tokens_to_nchw(dev(x), e(B, Cc, Hp << L, Wp << L, dtype=dtype), B, Hp, Wp, L)
        assert torch.equal(f5.cpu(), f.cpu())
        assert torch.equal(ops.nchw_to_tokens(ARENA.frozen(f5), e(x.shape[0], Cc), B, Hp, Wp, L).cpu(), x)


@pytest.mark.parametrize("dtype", DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,Hp,Wp", [(1, 2, 2), (1, 2, 4), (1, 3, 5), (3, 14, 18), (1, 10, 26)])      # 1, 2, 2 (odd grid: last row / column dropped), 63 x 3, 65 pooled positions
@pytest.mark.parametrize("Cc", [4, 1028])
def test_maxpool_tokens_edge_grids(ops, dtype, B, Hp, Wp, Cc):
    Ho, Wo = Hp // 2, Wp // 2
    x = rnd(B * Hp * Wp, Cc)
    if Hp * Wp > 5:
        x[5] = x[4]   # a tie: the gradient goes to the first maximum
    y = ops.maxpool2_tokens_fwd(dev(x), e(B * Ho * Wo, Cc, dtype=dtype), B, Hp, Wp)
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(O.tokens_to_nchw(xr, B, Hp, Wp, 0), 2, 2)
    assert torch.equal(y.float().cpu(), O.nchw_to_tokens(ref, B, Ho, Wo, 0).detach().to(dtype).float())
    dy = rnd(B * Ho * Wo, Cc, dtype=dtype, seed=2)
    ref.backward(O.tokens_to_nchw(dy, B, Ho, Wo, 0))
    dx = ops.maxpool2_tokens_bwd(dev(x), dev(dy, dtype), e(B * Hp * Wp, Cc), B, Hp, Wp)
    assert torch.equal(dx.cpu(), xr.grad)
    base = rnd(B * Hp * Wp, Cc, seed=3)
    dx2 = ops.maxpool2_tokens_bwd(dev(x), dev(dy, dtype), io(base), B, Hp, Wp, accumulate=True)
    assert rel_err(dx2.cpu(), base.double() + xr.grad.double()) < 1e-6


def test_layout_ops_refuse_channels_off_four(ops):
    """tokens_to_nchw / nchw_to_tokens / maxpool take channels in fours: C = 2 comes back as MTP_ERR_ARG and nothing is written"""
    x = dev(rnd(6, 2))
    out = ARENA.wide(1, 12)                                              # no column registered: all of it must stay poison
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_tokens_to_nchw"):
        ops.tokens_to_nchw(x, out.view(1, 2, 2, 3), 1, 2, 3, 0)
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_nchw_to_tokens"):
        ops.nchw_to_tokens(dev(rnd(1, 2, 2, 3)), out.view(6, 2), 1, 2, 3, 0)
    with pytest.raises(RuntimeError, match=ERR_ARG % "mtp_maxpool2_tokens_fwd"):
        ops.maxpool2_tokens_fwd(dev(rnd(24, 2)), out.view(6, 2), 1, 4, 6)
    torch.cuda.synchronize()
    ARENA.check()


# ------------------------------------------------------------------------------------------------ decode-head ops
def _rows(x, dtype=F32):
    return dev(x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]), dtype)


def _nchw(r, N, H, W):
    return r.float().cpu().reshape(N, H, W, -1).permute(0, 3, 1, 2)


def bn_case(rows, Cc, ref_dtype=torch.float64):
    """inputs of the BatchNorm edge test and the reference ReLU(BatchNorm(x)) with its input gradient, evaluated in ref_dtype by autograd"""
    g = torch.Generator().manual_seed(rows + Cc)
    x = torch.randn(rows, Cc, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    dy = torch.randn(rows, Cc, generator=g)
    xr = x.to(ref_dtype).requires_grad_(True)
    xh = (xr - xr.mean(0)) * (xr.var(0, unbiased=False) + 1e-5).rsqrt()
    pre = xh * gam.to(ref_dtype) + bet.to(ref_dtype)
    y_ref = F.relu(pre)
    y_ref.backward(dy.to(ref_dtype))
    return x, gam, bet, dy, pre.detach(), y_ref.detach(), xr.grad


def bn_dx_small_rows_bound(x, gam, dy):
    """one or two rows: xhat is 0 resp. +-1 up to eps / var, and dx = gamma rstd (dy' - mean(dy') - xhat mean(dy' xhat)) cancels to (almost) nothing --
    the result is orders of magnitude below its terms, so the f32 rounding of the TERMS (a few 2^-24 of gamma rstd |dy|) is what an f32 evaluation can
    promise: the error is bounded by 1e-4 of that scale, not of the cancelled result.  test_edge_bounds_host.py confirms on the CPU that a float32
    evaluation of the float64 reference stays inside this bound for the very inputs of the GPU test"""
    var = x.double().var(0, unbiased=False)
    return 1e-4 * float((gam.double() * (var + 1e-5).rsqrt() * dy.double().abs()).max())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("Cc", [4, 1024])
def test_batchnorm_edge_rows(ops, rows, Cc):
    x, gam, bet, dy, pre, y_ref, dx_ref = bn_case(rows, Cc)
    xd, dyd, gd, bd = dev(x), dev(dy), dev(gam), dev(bet)
    mean, rstd, center = e(Cc), e(Cc), e(Cc)
    ops.bn_finalize(ops.bn_sums(xd), rows, None, None, center, rstd)
    ops.bn_finalize(ops.bn_sums(xd, center), rows, None, None, mean, rstd, center=center)
    mu, var = x.double().mean(0), x.double().var(0, unbiased=False)
    assert rel_err(mean.cpu(), mu) < 1e-5 and rel_err(rstd.cpu(), (var + 1e-5).rsqrt()) < 1e-5
    y = ops.bn_apply(xd, mean, rstd, gd, bd, e(rows, Cc))
    assert rel_err(y.cpu(), y_ref) < 1e-5
    wide = ARENA.wide(rows, 3 * Cc, dtype=BF16)                         # into a column slice of a wider bf16 buffer (the concatenation)
    ops.bn_apply(xd, mean, rstd, gd, bd, ARENA.cols(wide, Cc, 2 * Cc))
    assert rel_err(wide[:, Cc:2 * Cc].float().cpu(), y_ref) < 8e-3
    bs = ops.bn_bwd_sums(dyd, xd, mean, rstd, gd, bd)
    dx = ops.bn_bwd_dx(dyd, xd, mean, rstd, gd, bd, bs, rows, e(rows, Cc))
    far = (pre.abs() > 1e-5).double()                                   # away from the ReLU's kink (see test_hip_uper_head)
    if rows >= 63:
        assert rel_err(dx.cpu() * far, dx_ref * far) < 1e-4
    else:
        assert float(((dx.cpu().double() - dx_ref) * far).abs().max()) < bn_dx_small_rows_bound(x, gam, dy)


@pytest.mark.parametrize("src,dst,N", [((1, 1), (1, 1), 1), ((1, 1), (1, 2), 1), ((1, 2), (7, 9), 1), ((9, 7), (1, 1), 2), ((5, 13), (2, 1), 1), ((3, 3), (5, 13), 1)])
@pytest.mark.parametrize("Cc", [4, 1024])
def test_resize_bilinear_edge_grids(ops, src, dst, N, Cc):
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    x = torch.randn(N, Cc, *src, generator=g, dtype=torch.float64, requires_grad=True)
    y_ref = F.interpolate(x, size=dst, mode="bilinear", align_corners=False)
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)
    y = ops.resize_bilinear_fwd(_rows(x.detach()), e(N * dst[0] * dst[1], Cc), N, *src, *dst)
    assert rel_err(_nchw(y, N, *dst), y_ref.detach()) < 1e-5
    dx = ops.resize_bilinear_bwd(_rows(dy), e(N * src[0] * src[1], Cc), N, *src, *dst)
    assert rel_err(_nchw(dx, N, *src), x.grad) < 1e-5
    wide = ARENA.wide(N * dst[0] * dst[1], 3 * Cc, dtype=BF16)
    mid = ARENA.cols(wide, Cc, 2 * Cc)
    mid.fill_(1.0)
    ops.resize_bilinear_fwd(_rows(x.detach(), BF16), mid, N, *src, *dst, accumulate=True)
    assert rel_err(_nchw(mid.contiguous(), N, *dst), y_ref.detach() + 1.0) < 1e-2


@pytest.mark.parametrize("H,W,S,N", [(1, 1, 1, 1), (1, 2, 1, 1), (7, 9, 1, 1), (5, 13, 2, 1), (1, 1, 3, 2), (7, 9, 6, 1)])
@pytest.mark.parametrize("Cc", [4, 1024])
def test_adaptive_avg_pool_edge_grids(ops, H, W, S, N, Cc):
    g = torch.Generator().manual_seed(H * 10 + S)
    x = torch.randn(N, Cc, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y_ref = F.adaptive_avg_pool2d(x, S)
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    y_ref.backward(dy)
    y = ops.adaptive_avg_pool_fwd(_rows(x.detach()), e(N * S * S, Cc), N, H, W, S)
    assert rel_err(_nchw(y, N, S, S), y_ref.detach()) < 1e-5
    dx = ops.adaptive_avg_pool_bwd(_rows(dy), e(N * H * W, Cc), N, H, W, S)
    assert rel_err(_nchw(dx, N, H, W), x.grad) < 1e-5


@pytest.mark.parametrize("N,h,w,K,label_dtype", [(1, 1, 1, 2, torch.uint8), (1, 1, 2, 8, torch.int64), (1, 7, 9, 3, torch.uint8), (1, 5, 13, 19, torch.int64), (2, 1, 1, 150, torch.uint8)])
def test_seg_ce_edge_grids(ops, N, h, w, K, label_dtype):
    from test_uper_head import torch_seg_loss
    g = torch.Generator().manual_seed(N + h + K)
    H, W = 4 * h, 4 * w
    logits = torch.randn(N, K, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    lab = torch.randint(0, K, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < 0.2] = 255
    lab[0, 0, 0] = 0
    ref = torch_seg_loss(logits, lab, 255, 0.7)
    ref.backward()
    Kp = ops.pad8(K)
    lr = torch.zeros(N * h * w, Kp)
    lr[:, :K] = logits.detach().permute(0, 2, 3, 1).reshape(-1, K).float()
    loss, dl = ops.seg_ce(dev(lr), K, N, h, w, dev(lab.to(label_dtype)), 255, 0.7)
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert rel_err(_nchw(dl[:, :K].contiguous(), N, h, w), logits.grad) < 1e-4
    # contract: the kernel writes only the K class columns of dlogits; with a padded row stride (ld = pad8(K) != K) it leaves the pad columns unwritten,
    # and the wrapper zeroes the buffer first (it comes from ops._scratch, i.e. poisoned here) so that the GEMM that consumes it reads zeros there
    assert Kp == K or dl[:, K:].abs().max().item() == 0.0
