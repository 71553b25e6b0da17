"""CPU: what tests/test_hip_sampling_edges.py takes for granted about its own inputs and bounds, asserted on the very inputs of the GPU tests
(tests/sampling_cases.py): the three statements of the window geometry agree on every grid; the float64 pooling reference equals torch's pad + AvgPool2d;
every avg element is constructed (and is what its construction says) or lies KINK away from 0, and KINK leaves the avg bound far behind; a float32
evaluation of every operator stays within HALF of its bound (no T of the table had to be raised); every named seam value lands on the branch it is named
for; the exact-sum inputs keep every partial sum below 2^24; and the thinned tables use every listed value."""
import pytest
import torch
import torch.nn.functional as F

import sampling_cases as S
from oracle.index_ops import rvsa_geometry

F32, BF16 = S.F32, S.BF16
CASES = S.sampling_cases()
EXTRA = [(1, 1, 1, S.C_MAX, 5, True), (1, 1, 1, 4, S.N_MAX, True)]      # the widest forward, the most heads of the backward


def within(got, ref, bound, what):
    err = (got.double() - ref.double()).abs()
    assert bool((err <= bound).all()), "%s: worst |err| / bound = %.3g" % (what, float((err / bound.clamp_min(1e-300)).max()))


def half(bound):
    return 0.5 * bound


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("Hp,Wp", S.GRIDS)
def test_the_three_statements_of_the_window_geometry_agree(Hp, Wp):
    from mtp_amd import ops
    pt, pl, nh, nw = S.windows(Hp, Wp)
    g = rvsa_geometry(Hp, Wp)
    assert ops.rvsa_windows(Hp, Wp) == (nh, nw) == (g["nh"], g["nw"]) and (pt, pl) == (g["pad_top"], g["pad_left"])
    assert 0 <= g["pad_down"] - pt <= 1 and 0 <= g["pad_right"] - pl <= 1 and g["pad_down"] <= 3 and g["pad_right"] <= 3      # the odd row / column is at the bottom / right
    tw = S.token_windows(2, Hp, Wp)
    assert sorted(set(tw.tolist())) == list(range(2 * nh * nw))          # every window holds a token: the clamp of a pad position stays inside it


def test_the_named_grids_are_what_their_names_say():
    assert S.windows(1, 1) == (3, 3, 1, 1)                  # one window, 48 pad positions
    assert S.windows(7, 7) == (0, 0, 1, 1)                  # no padding
    assert S.windows(8, 8) == (3, 3, 2, 2)                  # six pad rows and columns
    assert S.windows(1, 13) == (3, 0, 1, 2) and S.windows(13, 1) == (0, 3, 2, 1)      # pad = 1: nothing in front, only the far side is padded
    assert S.windows(6, 15) == (0, 3, 1, 3) and S.windows(14, 14) == (0, 0, 2, 2)
    # 8 x 8: the bottom window row / right window column reach row 0 / column 0 only through a clamp to 0 (the regime of the infinite token)
    tw = S.token_windows(1, 8, 8).view(8, 8)
    assert tw[0, 0] == 0 and set(tw[0].tolist()) == {0, 1} and set(tw[:, 0].tolist()) == {0, 2}


@pytest.mark.parametrize("Hp,Wp", S.GRIDS)
def test_pool_reference_is_torchs_pad_and_avgpool(Hp, Wp):
    B, Cc = 3, 8
    x = S.rnd(B * Hp * Wp, Cc, seed=3)
    g = rvsa_geometry(Hp, Wp)
    img = x.double().view(B, Hp, Wp, Cc).permute(0, 3, 1, 2)
    ref = F.avg_pool2d(F.pad(img, (g["pad_left"], g["pad_right"], g["pad_top"], g["pad_down"])), 7, 7).permute(0, 2, 3, 1).reshape(-1, Cc)
    avg, mag = S.pool_ref(x, B, Hp, Wp)
    assert float((avg - ref).abs().max()) <= 1e-15 and bool((mag >= avg.abs() - 1e-15).all())
    assert torch.equal(S.slope_of(torch.tensor([0.0, -0.0, 1.0, -1.0])), torch.tensor([0.01, 0.01, 1.0, 0.01], dtype=torch.float64))
    z = torch.tensor([0.0, -0.0], requires_grad=True)
    F.leaky_relu(z, 0.01).sum().backward()
    assert z.grad.tolist() == [pytest.approx(0.01)] * 2       # torch's LeakyReLU backward at 0.0 and -0.0


# ------------------------------------------------------------------------------------------------ kink
@pytest.mark.parametrize("case", CASES + EXTRA, ids=S.case_id)
def test_every_average_is_constructed_or_kink_away_from_zero(case):
    Hp, Wp, B, Cc, N, bias = case
    c = S.sampling_case(*case)
    x, tw = c["x"], c["tw"]
    assert torch.equal(x.to(BF16).float(), x) and all(torch.equal(c[k].to(BF16).float(), c[k]) for k in ("w", "dsamp", "dpooled", "base"))
    made = S.made_mask(c["R"], Cc)
    assert float(c["avg"][~made].abs().min()) >= S.KINK if bool((~made).any()) else True
    assert S.KINK >= 16 * float(S.sum_bound(50, c["avgmag"], c["avg"]).max())
    # the constructed window-channels
    t0 = (tw == 0).nonzero().reshape(-1)
    x0 = x[t0, :S.MADE]
    assert float(x0[:, 0].abs().max()) == 0 and float(x0[:, 3].abs().max()) == 0 and bool(torch.signbit(x0[:, 3]).all())
    assert x0[0, 1] == -S.TINY and x0[0, 2] == S.TINY and float(x0[1:, 1:3].abs().sum()) == 0
    assert c["avg"][0, :S.MADE].tolist() == [0.0, -S.TINY / 49, S.TINY / 49, 0.0]
    assert c["avg_made"].tolist()[0::3] == [0.0, 0.0] and c["pooled_made"][1] < 0 < c["pooled_made"][2]
    # backward: avg is an input -- 0.0, -0.0, +-2^-20 / 49 in window 0, the rest KINK away
    a = c["avg_in"]
    assert a[0, 0] == 0 and not bool(torch.signbit(a[0, 0])) and a[0, 1] == 0 and bool(torch.signbit(a[0, 1])) and a[0, 2] > 0 > a[0, 3]
    assert c["slope_in"][0, :S.MADE].tolist() == [0.01, 0.01, 1.0, 0.01]
    assert float(a[~made].abs().min()) >= 0.99 * S.KINK if bool((~made).any()) else True
    assert (c["b"] is None) == (not bias)


# ------------------------------------------------------------------------------------------------ half of every bound
@pytest.mark.parametrize("case", CASES + EXTRA, ids=S.case_id)
def test_float32_sampling_heads_stay_within_half_of_every_bound(case):
    Hp, Wp, B, Cc, N, _ = case
    c = S.sampling_case(*case)
    R, tw, T = c["R"], c["tw"], S.TERMS
    k = torch.tensor(1.0) / torch.tensor(49.0)
    avg = torch.zeros(R, Cc).index_add_(0, tw, c["x"]) * k
    pooled = torch.where(avg > 0, avg, torch.tensor(0.01) * avg)
    within(avg, c["avg"], half(S.sum_bound(T["avg"](Cc, N), c["avgmag"], c["avg"])), "avg")
    within(pooled, c["pooled"], half(S.sum_bound(T["pooled"](Cc, N), c["pooledmag"], c["pooled"])), "pooled")
    assert torch.equal(avg[0, :S.MADE], c["avg_made"]) and torch.equal(pooled[0, :S.MADE], c["pooled_made"])
    ref, mag = S.samp_ref(pooled, c["w"], c["b"])
    samp = pooled @ c["w"].t() + (c["b"] if c["b"] is not None else 0.0)
    within(samp, ref, half(S.sum_bound(T["samp"](Cc, N), mag, ref)), "samp")
    fac = torch.where(c["avg_in"] > 0, k, torch.tensor(0.01) * k)
    g = (c["dsamp"] @ c["w"]) * fac
    within(g, c["g"], half(S.sum_bound(T["g"](Cc, N), c["gmag"], c["g"])), "g")
    base = c["base"].double()
    for name, add, addmag in (("sampling_dx", g[tw], c["gmag"][tw]), ("pool_dx", (c["dpooled"] * fac)[tw], c["pg"][tw].abs())):
        want = c["g"][tw] if name == "sampling_dx" else c["pg"][tw]
        f32b = S.sum_bound(T[name](Cc, N), base.abs() + addmag, base + want)
        within(c["base"] + add, base + want, half(f32b), name)
        # (a bf16 output: the 2^-8 |ref| term IS the worst rounding of an 8-bit significand -- room only in the f32 part)
        within((c["base"] + add).to(BF16), base + want, half(f32b) + 2.0 ** -8 * (base + want).abs(), name + " bf16")
    within(c["dpooled"] * fac, c["pg"], half(S.sum_bound(T["pool_dx"](Cc, N), c["pg"].abs(), c["pg"])), "pool_dx, no accumulation")


@pytest.mark.parametrize("R,N,K", S.small_linear_cases())
def test_float32_small_linear_stays_within_half_of_every_bound(R, N, K):
    c = S.linear_case(R, N, K, False)
    x, w, b, dy = c["x"], c["w"], c["b"], c["dy"]
    within(x @ w.t() + b, c["y"], half(S.sum_bound(K + 1, c["ymag"], c["y"])), "y")
    within(dy @ w, c["dx"], half(S.sum_bound(N, c["dxmag"], c["dx"])), "dx")
    within(dy.t() @ x, c["dw"], half(S.sum_bound(R, c["dwmag"], c["dw"])), "dw")
    within(dy.sum(0), c["db"], half(S.sum_bound(R, c["dbmag"], c["db"])), "db")


def check_float32_segments(c, R, rows, bw, bb):
    """dw[j] and db[j] of every segment, accumulated in float32 onto the starting values the GPU test uses, within half of the bound"""
    dw, db, r0 = c["dy"].t() @ c["x"], c["dy"].sum(0), 0
    for j, r in enumerate(rows):
        sl = slice(r0, r0 + r)
        ref = bw[j].double() + c["dw"][sl]
        within(bw[j] + dw[sl], ref, half(S.sum_bound(R, bw[j].double().abs() + c["dwmag"][sl], ref)), "dw[%d] +=" % j)
        if bb[j] is not None:
            ref = bb[j].double() + c["db"][sl]
            within(bb[j] + db[sl], ref, half(S.sum_bound(R, bb[j].double().abs() + c["dbmag"][sl], ref)), "db[%d] +=" % j)
        r0 += r


@pytest.mark.parametrize("R,K,rows,has_db", S.segment_cases(), ids=S.case_id)
def test_float32_segments_stay_within_half_of_the_bound_with_their_starting_values(R, K, rows, has_db):
    assert 1 <= len(rows) <= 4 and len(has_db) == len(rows)
    bw, bb = S.seg_buffers(rows, has_db, K, False)
    assert [t is not None for t in bb] == list(has_db) and [t.shape[0] for t in bw] == list(rows)
    check_float32_segments(S.linear_case(R, sum(rows), K, False), R, rows, bw, bb)


@pytest.mark.parametrize("i", range(S.SL_BATCH))
def test_float32_batched_problems_stay_within_half_of_the_bound(i):
    c, (bw, bb) = S.batched_problem(i, False)
    check_float32_segments(c, S.BATCHED["R"], S.BATCHED["rows"], bw, bb)
    assert i == 0 or not torch.equal(c["x"], S.batched_problem(0, False)[0]["x"])          # another problem, not the same one again


# ------------------------------------------------------------------------------------------------ exact sums
LIMIT = 2.0 ** 24


@pytest.mark.parametrize("R,N,K", S.small_linear_cases() + [(S.DX_ROWS_MAX, 1, 4)] + sorted({(R, sum(rows), K) for R, K, rows, _ in S.segment_cases()}) + [(S.BATCHED["R"], sum(S.BATCHED["rows"]), S.BATCHED["K"])])
def test_exact_sum_inputs_stay_below_2_to_the_24(R, N, K):
    """sum|terms| bounds every partial sum, in whatever order the kernel and its atomics add; + 4 for a starting value (segments) or the bias"""
    for salt in range(S.SL_BATCH + 1):
        c = S.linear_case(R, N, K, True, salt)
        for k in ("x", "w", "b", "dy"):
            assert float(c[k].abs().max()) <= 4 and torch.equal(c[k], c[k].round())
        for k in ("ymag", "dxmag", "dwmag", "dbmag"):
            assert float(c[k].max()) + 4 < LIMIT
        assert torch.equal((c["x"] @ c["w"].t() + c["b"]).double(), c["y"]) and torch.equal((c["dy"].t() @ c["x"]).double(), c["dw"])
        if (R, N, K) != (S.BATCHED["R"], sum(S.BATCHED["rows"]), S.BATCHED["K"]):
            break       # only the batched test uses further problems of a shape
        if salt:
            assert c is S.batched_problem(salt - 1, True)[0]
            for t in S.batched_problem(salt - 1, True)[1][0]:
                assert float(t.abs().max()) <= 4 and torch.equal(t, t.round())


# ------------------------------------------------------------------------------------------------ seams
# Which branch a size takes: each function restates the line of mtp_amd/csrc named in RESTATES, and test_restated_lines_are_where_they_are_said_to_be
# reads that line, so an edit of the kernels that moves or changes one of them fails here instead of leaving a restatement behind.
def fwd_variant(K):
    """mtp_small_linear_fwd: <ROWS 4, MAXJ 4> up to K = 1024, <2, 8> up to 2048, else the generic kernel"""
    return "r4j4" if K <= 1024 else ("r2j8" if K <= 2048 else "generic")


def ysplit(N):
    """mtp_rvsa_sampling_fwd: workgroups per window"""
    return 2 if N >= 32 else 1


def head_share(N):
    """rvsa_sampling_fwd_kernel: [nlo, nhi) of each workgroup of a window -- the share is rounded up to a multiple of four"""
    y = ysplit(N)
    nper = ((N + y - 1) // y + 3) // 4 * 4
    return [(i * nper, min(i * nper + nper, N)) for i in range(y)]


def zsplit(R):
    """the dw kernels: 4 waves x SL_DW_ROWS = 128 rows per workgroup in z"""
    return (R + 127) // 128


def yblocks(C):
    """the backward grids: 64 channel quads per workgroup in y"""
    return (C // 4 + 63) // 64


def ktrips(C):
    """rvsa_heads: trips of the forward's k loop, 4 steps of 256 floats each; the last one masked where C is no multiple of 1024"""
    return (C + 1023) // 1024


def dx_xblocks(K):
    """mtp_small_linear_bwd: workgroups in x of small_linear_dx, 1024 columns each"""
    return (K + 1023) // 1024


def dw_groups(N, K):
    """the dw grids: (256-column groups in x, 8-output groups in y)"""
    return (K + 255) // 256, (N + 7) // 8


def wave_quarter(N):
    """small_linear_fwd_kernel: [n_lo, n_hi) of each of the 4 waves"""
    per = (N + 3) // 4
    return [(min(v * per, N), min(v * per + per, N)) for v in range(4)]


RESTATES = [      # (restatement, file under mtp_amd/csrc, line, what that line holds)
    (fwd_variant, "rvsa_sampling.hip", 399, "if (K <= 1024)"),
    (fwd_variant, "rvsa_sampling.hip", 401, "else if (K <= 2048)"),
    (ysplit, "rvsa_sampling.hip", 357, "constexpr int ysplit = 2;"),
    (ysplit, "rvsa_sampling.hip", 358, "(unsigned)(N >= 16 * ysplit ? ysplit : 1)"),
    (head_share, "rvsa_sampling.hip", 275, "const int nper = ((N + (int)gridDim.y - 1) / (int)gridDim.y + 3) / 4 * 4, nlo = (int)blockIdx.y * nper, nhi = (nlo + nper) < N ? (nlo + nper) : N;"),
    (zsplit, "rvsa_sampling.hip", 259, "return (R + 4 * SL_DW_ROWS - 1) / (4 * SL_DW_ROWS);"),
    (zsplit, "rvsa_sampling.hip", 156, "constexpr int SL_DW_ROWS = 32;"),
    (yblocks, "rvsa_sampling.hip", 345, "(unsigned)((C / 4 + 63) / 64)"),
    (yblocks, "rvsa_sampling.hip", 370, "(unsigned)((C / 4 + 63) / 64)"),
    (ktrips, "rvsa_sampling_body.h", 67, "for (int k0 = lane * 4; k0 < C; k0 += 1024) {"),
    (dx_xblocks, "rvsa_sampling.hip", 411, "small_linear_dx_kernel<<<dim3((unsigned)((K + 1023) / 1024), (unsigned)((R + 3) / 4))"),
    (dw_groups, "rvsa_sampling.hip", 419, "const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((N + 7) / 8), (unsigned)sl_dw_zsplit(R));"),
    (dw_groups, "rvsa_sampling.hip", 441, "const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((N + 7) / 8), (unsigned)sl_dw_zsplit(R));"),
    (wave_quarter, "rvsa_sampling.hip", 95, "const int per = (N + 3) / 4, n_lo = wave * per, n_hi = (n_lo + per) < N ? (n_lo + per) : N;"),
]


@pytest.mark.parametrize("fn,name,line,text", RESTATES, ids=["%s-%s:%d" % (r[0].__name__, r[1], r[2]) for r in RESTATES])
def test_restated_lines_are_where_they_are_said_to_be(fn, name, line, text):
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mtp_amd", "csrc", name)
    with open(path) as f:
        got = f.read().split("\n")[line - 1]
    assert text in got, "%s:%d no longer holds what %s restates: %r" % (name, line, fn.__name__, got.strip())


def test_named_seam_values_land_on_their_branches():
    # small_linear_fwd by K
    assert [fwd_variant(K) for K in S.SL_K] == ["r4j4"] * 5 + ["r2j8"] * 2 + ["generic"]
    # 256-column groups of dw, dx's second x block
    assert [dw_groups(8, K)[0] for K in (252, 256, 260)] == [1, 1, 2] and [dx_xblocks(K) for K in (1024, 1028, 2052)] == [1, 2, 3]
    # rows: groups of 4 and of 2, a wave's 32 rows, the 128-row z split
    assert [zsplit(R) for R in (127, 128, 129, 257)] == [1, 1, 2, 3]
    assert {R % 4 for R in S.SL_R} == {0, 1, 2, 3} and {31, 32, 33} <= set(S.SL_R)
    # outputs: the forward's wave quarters (N < 4 leaves waves empty; 5, 7, 9, 83 end on a ragged pass of 4), the 8-output groups of dw
    assert wave_quarter(1) == [(0, 1), (1, 1), (1, 1), (1, 1)] and wave_quarter(5) == [(0, 2), (2, 4), (4, 5), (5, 5)]
    assert wave_quarter(83)[3] == (63, 83) and wave_quarter(80)[3] == (60, 80)
    assert [dw_groups(N, 4)[1] for N in (7, 8, 9, 80, 83)] == [1, 1, 2, 10, 11]
    # the fused forward: one -> two workgroups per window, each share a multiple of four
    assert [ysplit(N) for N in (31, 32, 33)] == [1, 2, 2]
    assert head_share(31) == [(0, 31)] and head_share(32) == [(0, 16), (16, 32)] and head_share(33) == [(0, 20), (20, 33)]
    assert head_share(60) == [(0, 32), (32, 60)] and head_share(83) == [(0, 44), (44, 83)]
    for N in S.HEADS:
        sh = head_share(N)
        assert sh[0][0] == 0 and sh[-1][1] == N and all(a[1] == b[0] for a, b in zip(sh, sh[1:])) and all(a % 4 == 0 for a, _ in sh)
    # the masked second trip of the forward's k loop; the 64-quad split of the backward grids
    assert [ktrips(Cc) for Cc in (1024, 1028, 1280, S.C_MAX)] == [1, 2, 2, 8]
    assert [yblocks(Cc) for Cc in (4, 252, 256, 260, 1280)] == [1, 1, 1, 2, 5]
    assert S.DX_ROWS_MAX == 262140 and (S.DX_ROWS_MAX + 3) // 4 == 65535 and (S.DX_ROWS_MAX + 1 + 3) // 4 == 65536


def test_entry_points_refuse_sizes_their_kernels_cannot_hold():
    """the argument checks run before any launch and dereference nothing, so they are testable without a device, and at sizes no test could allocate:
    a size of 0, a size no int holds (R, N, K, C, Hp, Wp, the window count), K = 0 (it passes K % 4; the forward's clamped weight index would be -1),
    and a row count beyond what the y dimension of small_linear_dx's grid takes.  P: non-NULL, 16-byte aligned, never dereferenced."""
    import ctypes as C
    from mtp_amd import _lib
    lib = _lib.load()
    P, BIG, F32 = 1 << 20, 2 ** 31 - 1, _lib.MTP_F32
    for s in [(0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (1, 8, 8, 6), (1, BIG, 8, 8), (1, 8, BIG, 8), (1, 8, 8, BIG + 1), (BIG, 8, 8, 8),
              (2 ** 29, 14, 14, 8), (1, 2 ** 20 * 7, 2 ** 20 * 7, 8),
              (1, 2 ** 15 * 7, 2 ** 15 * 7, 2 ** 30)]:      # (the last: 2^30 windows, but 49 * 2^30 tokens x 2^30 channels overflow the int64 element count)
        assert lib.mtp_rvsa_pool_fwd(P, F32, P, P, *s, None) == -1, s
        assert lib.mtp_rvsa_pool_bwd(P, P, P, F32, 0, *s, None) == -1, s
        assert lib.mtp_rvsa_sampling_fwd(P, F32, P, P, P, P, P, *s, 4, None) == -1, s
        assert lib.mtp_rvsa_sampling_bwd(P, P, P, P, F32, *s, 4, None) == -1, s
    assert lib.mtp_rvsa_sampling_fwd(P, F32, P, P, P, P, P, 1, 8, 8, S.C_MAX + 4, 4, None) == -1
    assert lib.mtp_rvsa_sampling_fwd(P, F32, P, P, P, P, P, 1, 8, 8, 8, BIG, None) == -1
    assert lib.mtp_rvsa_sampling_bwd(P, P, P, P, F32, 1, 8, 8, 8, S.N_MAX + 1, None) == -1
    for s in [(0, 8, 4), (BIG, 8, 4), (4, 0, 4), (4, BIG + 1, 4), (4, 8, 0), (4, 8, S.N_MAX + 1)]:
        assert lib.mtp_rvsa_sampling_bwd_win(P, P, P, P, *s, None) == -1, s
    rows, ptrs = (C.c_int64 * 2)(4, 4), (C.c_void_p * 2)(P, P)
    for s in [(0, 8, 8), (5, 0, 8), (5, 8, 0), (5, 8, 6), (BIG, 8, 8), (5, BIG, 8), (5, 8, BIG + 1), (5, 8, -4)]:
        assert lib.mtp_small_linear_fwd(P, P, P, P, *s, None) == -1, s
        assert lib.mtp_small_linear_bwd(P, P, P, P, P, P, *s, None) == -1, s
        assert lib.mtp_small_linear_dw_segments(P, P, *s, 2, rows, ptrs, ptrs, None) == -1, s
        assert lib.mtp_small_linear_dw_segments_batched(ptrs, ptrs, 1, *s, 2, rows, ptrs, ptrs, None) == -1, s
    assert lib.mtp_small_linear_bwd(P, P, P, P, None, None, S.DX_ROWS_MAX + 1, 8, 8, None) == -1          # dx: grid.y = 65536
    assert lib.mtp_small_linear_bwd(P, P, P, None, P, P, 128 * 65535 + 1, 8, 8, None) == -1               # dw: grid.z = 65536
    assert lib.mtp_small_linear_dw_segments(P, P, 128 * 65535 + 1, 8, 8, 2, rows, ptrs, ptrs, None) == -1
    assert lib.mtp_small_linear_dw_segments_batched(ptrs, ptrs, 2, 128 * 32768, 8, 8, 2, rows, ptrs, ptrs, None) == -1      # 2 problems x 32768 row parts
    for nseg, count in [(0, 1), (5, 1), (2, 0), (2, S.SL_BATCH + 1)]:
        assert lib.mtp_small_linear_dw_segments_batched(ptrs, ptrs, count, 5, 8, 8, nseg, rows, ptrs, ptrs, None) == -1
    assert lib.mtp_small_linear_dw_segments(P, P, 5, 8, 8, 2, (C.c_int64 * 2)(4, 3), ptrs, ptrs, None) == -1


def test_thinned_tables_use_every_listed_value():
    cs = CASES
    assert {(c[0], c[1], c[2]) for c in cs} == {(h, w, b) for h, w in S.GRIDS for b in S.BATCHES}
    assert {c[3] for c in cs} == set(S.WIDTHS) and {c[4] for c in cs} == set(S.HEADS) and sum(1 for c in cs if not c[5]) == 1
    sl = S.small_linear_cases()
    assert {c[0] for c in sl} >= set(S.SL_R) and {c[1] for c in sl} == set(S.SL_N) and {c[2] for c in sl} == set(S.SL_K)
    assert max(r * n * k for r, n, k in sl) == 257 * 83 * 2052
    seg = S.segment_cases()
    assert {len(c[2]) for c in seg} == {1, 2, 3, 4} and any(not all(c[3]) for c in seg)
    assert any(any((sum(c[2][:j]) % 8) for j in range(1, len(c[2]))) for c in seg)          # a segment starts inside an 8-output group
