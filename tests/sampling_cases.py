"""Case tables and float64 references of the RVSA sampling heads (csrc/rvsa_sampling.hip, csrc/rvsa_sampling_body.h), shared by
tests/test_hip_sampling_edges.py (GPU) and tests/test_sampling_edges_host.py (CPU).  Plain torch on the CPU: no device, no library.

Every input holds values bf16 represents exactly, so one case serves the f32 and the bf16 run.  The references are float64, computed from those inputs;
each comes with the sum of the absolute values of its terms (`*mag`), the quantity the element-wise bound scales with:

    |got - ref| <= 2 T 2^-24 sum|terms|   [+ 2^-8 |ref| for a bf16 output]            (T: the table TERMS below)

LeakyReLU kink.  pooled, g and dx depend on the sign of avg.  Every avg element of a case is either constructed so that its sign is decided exactly
(window 0, channels 0 .. 3: all tokens 0.0 | one token -2^-20, the others 0 | one token +2^-20 | all tokens -0.0) or lies at least KINK from 0 in float64
(a window-channel whose random average falls below KINK gets +-1 added to its first token).  The backward kernels take avg as an input: there channels
0 .. 3 of window 0 hold 0.0, -0.0, +2^-20 / 49, -2^-20 / 49.
"""
import functools

import torch

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------ tables
GRIDS = [(1, 1), (7, 7), (8, 8), (1, 13), (13, 1), (6, 15), (14, 14)]
BATCHES = [1, 3]
WIDTHS = [4, 252, 256, 260, 1024, 1028, 1280]                    # 256 | 260: the 64-quad split of the backward grids; 1024 | 1028: the masked second trip of the forward's k loop
HEADS = [1, 3, 4, 5, 15, 16, 31, 32, 33, 60, 80, 83]             # 31 | 32 | 33: one -> two workgroups per window in the forward
C_MAX, N_MAX = 8192, 4096                                        # accepted by the forward / by the two backward entry points; + 4 / + 1 is refused
KINK = 2.0 ** -10         # >= 16 x the largest avg bound of any case, 2 * 50 * 2^-24 * sum|x| / 49 (test_sampling_edges_host.py asserts it)
TINY = 2.0 ** -20
MADE = 4                  # channels 0 .. 3 of window 0 are the constructed ones

SL_R = [1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129, 257]           # row groups of 4 and 2, a wave's 32 rows, the 128-row z split
SL_N = [1, 3, 4, 5, 7, 8, 9, 80, 83]                             # the wave quarter of the forward, the 8-output groups of dw
SL_K = [4, 252, 256, 260, 1024, 1028, 2048, 2052]                # <4, 4> | <2, 8> | generic forward, the 256-column groups of dw, dx's second x block
SL_BATCH = 8
DX_ROWS_MAX = 4 * 65535   # small_linear_dx: grid.y = ceil(R / 4)

# T of the bound, per output
TERMS = dict(avg=lambda C, N: 50, pooled=lambda C, N: 52, samp=lambda C, N: C + 1, g=lambda C, N: N + 2, sampling_dx=lambda C, N: N + 3,
             pool_dx=lambda C, N: 3)


def sampling_cases():
    """(Hp, Wp, B, C, N, bias): every grid with B = 1 and 3; the widths and head counts cycle through them, so every C and every N runs with every entry
    point; bias = None once; and N = 33 / 80 (two workgroups per window) once more at C = 1028 / 1280 (the masked trip, the model's widest)"""
    out, i = [], 0
    for Hp, Wp in GRIDS:
        for B in BATCHES:
            out.append((Hp, Wp, B, WIDTHS[i % len(WIDTHS)], HEADS[i % len(HEADS)], i != 5))
            i += 1
    return out + [(8, 8, 3, 1028, 33, True), (14, 14, 3, 1280, 80, True)]


def case_id(c):
    """id of a case tuple, or of one value of it where pytest asks per argument"""
    if not isinstance(c, (list, tuple)):
        return str(int(c))
    return "-".join(str(int(v)) if not isinstance(v, (list, tuple)) else "x".join(str(int(u)) for u in v) for v in c)


def small_linear_cases():
    """(R, N, K): every R, every N, every K, then the largest of each together and the seams that the cycle does not pair"""
    out = [(R, SL_N[i % len(SL_N)], SL_K[i % len(SL_K)]) for i, R in enumerate(SL_R)]
    return out + [(257, 83, 2052), (129, 80, 1028), (33, 7, 1024), (3, 5, 2048), (130, 9, 260)]


def segment_cases():
    """(R, K, rows per segment, which segments have a db): nseg 1 .. 4, rows that cross the 8-output groups"""
    return [(1, 4, (1,), (True,)), (33, 260, (3, 5, 1, 2), (True, False, True, True)), (129, 1028, (8, 8), (False, False)),
            (257, 256, (7, 9, 64), (True, True, False)), (5, 252, (80, 3), (True, True)), (128, 4, (32, 32, 16), (True, True, True))]


# ------------------------------------------------------------------------------------------------ geometry
def windows(Hp, Wp):
    """(pad_t, pad_l, nh, nw): restates RvsaWindows, csrc/common.h:241"""
    pad_h, pad_w = (7 - Hp % 7) % 7, (7 - Wp % 7) % 7
    return pad_h // 2, pad_w // 2, (Hp + pad_h) // 7, (Wp + pad_w) // 7


def token_windows(B, Hp, Wp):
    """(B * Hp * Wp,) int64: the window (b, i, j) -> (b * nh + i) * nw + j that holds each token"""
    pt, pl, nh, nw = windows(Hp, Wp)
    win = (((torch.arange(Hp) + pt) // 7)[:, None] * nw + ((torch.arange(Wp) + pl) // 7)[None, :]).reshape(-1)
    return (torch.arange(B)[:, None] * (nh * nw) + win[None, :]).reshape(-1)


# ------------------------------------------------------------------------------------------------ inputs
def rnd(*shape, seed=0, scale=1.0):
    """normal values that bf16 holds exactly, as float32"""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape) + 7 * len(shape))) * scale
    return t.to(BF16).float()


def ints(*shape, seed=0):
    """integers in [-4, 4] as float32: every f32 sum of their products is exact while it stays below 2^24"""
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed + sum(shape) + 7 * len(shape))).float()


def slope_of(avg):
    """LeakyReLU'(avg) as the kernels and torch have it: 1 where avg > 0, else 0.01 (at 0.0 and -0.0 too)"""
    return torch.where(avg > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.01, dtype=torch.float64))


def pool_ref(x, B, Hp, Wp):
    """float64 zero pad + AvgPool2d(7, 7) (always / 49): avg (windows, C) and sum|terms|"""
    tw = token_windows(B, Hp, Wp)
    _, _, nh, nw = windows(Hp, Wp)
    x = x.double()
    z = torch.zeros(B * nh * nw, x.shape[1], dtype=torch.float64)
    return z.clone().index_add_(0, tw, x) / 49.0, z.clone().index_add_(0, tw, x.abs()) / 49.0


def tokens(Hp, Wp, B, C, seed=0):
    """the token tensor of a case: random, pushed off the kink, with the constructed channels in window 0"""
    tw = token_windows(B, Hp, Wp)
    x = rnd(B * Hp * Wp, C, seed=seed)
    avg, _ = pool_ref(x, B, Hp, Wp)
    first = torch.full((int(tw.max()) + 1,), -1, dtype=torch.int64)
    for t in range(tw.numel() - 1, -1, -1):
        first[tw[t]] = t                                                  # the first token of every window
    near = avg.abs() < 2 * KINK
    push = torch.where(avg < 0, -1.0, 1.0).float() * near.float()           # +-1 / 49 = 0.02 onto the average
    x.index_add_(0, first, push)
    x = x.to(BF16).float()
    t0 = (tw == 0).nonzero().reshape(-1)
    x[t0, 0] = 0.0
    x[t0, 1] = 0.0
    x[t0[0], 1] = -TINY
    x[t0, 2] = 0.0
    x[t0[0], 2] = TINY
    x[t0, 3] = -0.0
    return x


def made_mask(R, C):
    m = torch.zeros(R, C, dtype=torch.bool)
    m[0, :MADE] = True
    return m


@functools.lru_cache(maxsize=None)
def sampling_case(Hp, Wp, B, C, N, bias=True):
    """inputs (float32, bf16-exact) and float64 references of one case; nothing in it is changed by a test"""
    pt, pl, nh, nw = windows(Hp, Wp)
    R, T = B * nh * nw, B * Hp * Wp
    seed = 1000 * Hp + 100 * Wp + 10 * B + C + N
    c = dict(R=R, T=T, tw=token_windows(B, Hp, Wp), geom=(pt, pl, nh, nw))
    c["x"] = x = tokens(Hp, Wp, B, C, seed)
    c["w"], c["b"] = rnd(N, C, seed=seed + 1, scale=0.1), (rnd(N, seed=seed + 2) if bias else None)
    c["avg"], c["avgmag"] = pool_ref(x, B, Hp, Wp)
    s = slope_of(c["avg"])
    c["pooled"], c["pooledmag"] = c["avg"] * s, c["avgmag"] * s
    # the exact values of the constructed elements: one rounding each, in float32
    k = torch.tensor(1.0) / torch.tensor(49.0)
    c["avg_made"] = torch.tensor([0.0, -TINY, TINY, 0.0]) * k
    c["pooled_made"] = torch.where(c["avg_made"] > 0, c["avg_made"], torch.tensor(0.01) * c["avg_made"])
    # backward: avg is an input
    avg_in = c["avg"].float()
    avg_in[0, :MADE] = torch.tensor([0.0, -0.0, TINY, -TINY]) * k
    c["avg_in"] = avg_in
    sb = c["slope_in"] = slope_of(avg_in)
    c["dsamp"], c["dpooled"], c["base"] = rnd(R, N, seed=seed + 3), rnd(R, C, seed=seed + 4), rnd(T, C, seed=seed + 5)
    c["g"], c["gmag"] = (c["dsamp"].double() @ c["w"].double()) * sb / 49.0, (c["dsamp"].double().abs() @ c["w"].double().abs()) * sb / 49.0
    c["pg"] = c["dpooled"].double() * sb / 49.0                     # pool_bwd's per-window addend
    return c


def samp_ref(pooled, w, b):
    """float64 heads of a pooled tensor (the device's own, read back): ref and sum|terms|"""
    p, w = pooled.double(), w.double()
    ref, mag = p @ w.t(), p.abs() @ w.abs().t()
    return (ref + b.double(), mag + b.double().abs()) if b is not None else (ref, mag)


def sum_bound(T, mag, ref, out_dtype=F32):
    b = 2.0 * T * U * mag.double()
    return b + 2.0 ** -8 * ref.double().abs() if out_dtype == BF16 else b


# ------------------------------------------------------------------------------------------------ small_linear
@functools.lru_cache(maxsize=None)
def linear_case(R, N, K, exact, salt=0):
    """x (R, K), w (N, K), b (N), dy (R, N) and the float64 results with their sum|terms|; exact: small integers, every sum an integer below 2^24;
    salt: another problem of the same shape"""
    f = ints if exact else rnd
    seed = 31 * R + 17 * N + K + 1000 * salt
    x, w, b, dy = f(R, K, seed=seed), f(N, K, seed=seed + 1), f(N, seed=seed + 2), f(R, N, seed=seed + 3)
    if not exact:
        w = (w * 0.125).to(BF16).float()
    X, W, Bv, D = x.double(), w.double(), b.double(), dy.double()
    c = dict(x=x, w=w, b=b, dy=dy, exact=exact)
    c["y"], c["ymag"] = X @ W.t() + Bv, X.abs() @ W.abs().t() + Bv.abs()
    c["y0"], c["y0mag"] = X @ W.t(), X.abs() @ W.abs().t()          # bias = None
    c["dx"], c["dxmag"] = D @ W, D.abs() @ W.abs()
    c["dw"], c["dwmag"] = D.t() @ X, D.abs().t() @ X.abs()
    c["db"], c["dbmag"] = D.sum(0), D.abs().sum(0)
    return c


def seg_buffers(rows, has_db, K, exact, salt=0):
    """the starting values of the segments' dw (rows_j, K) and db (rows_j; None where the segment has none): the calls accumulate onto them"""
    f = ints if exact else rnd
    bw = [f(r, K, seed=40 + 5 * salt + j) for j, r in enumerate(rows)]
    bb = [f(r, seed=60 + 5 * salt + j) if h else None for j, (r, h) in enumerate(zip(rows, has_db))]
    return bw, bb


# the batched form: R = 129 -> blockIdx.z = problem * 2 + row part, the last part one row long
BATCHED = dict(R=129, K=260, rows=(3, 5, 1, 2), has_db=(True, False, True, True))


def batched_problem(i, exact):
    """problem i of the batched call: its linear_case and its starting values"""
    b = BATCHED
    return linear_case(b["R"], sum(b["rows"]), b["K"], exact, i + 1), seg_buffers(b["rows"], b["has_db"], b["K"], exact, salt=i)
