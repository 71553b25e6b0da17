"""Thin torch-tensor wrappers over the C ABI (include/mtp_hip.h).  PyTorch is plumbing here: device memory,
the current HIP stream, nothing else.  Every function launches hand-written gfx950 kernels from libmtp_hip.so
on torch's current stream; there is no CPU / eager fallback -- CPU tensors raise.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_DG, EPI_BIAS_RES, EPI_DGELU, EPI_MUL, MTP_BF16, MTP_F32, GemmArgs,  # noqa: F401
                   check)
from ._lib import (GEMM_NT_FAMILY_P8, GEMM_NT_FAMILY_REG, GEMM_NT_FAMILY_SB, GEMM_NT_FAMILY_SB8, GEMM_NT_FAMILY_STRIP, GEMM_NT_NO_P8,  # noqa: F401
                   GEMM_NT_NO_PERSIST, GEMM_NT_NO_SB8, GEMM_NT_NO_STRIP, GEMM_NT_P8, GEMM_NT_P8_224, GEMM_NT_P8_256, GEMM_NT_PERSIST,
                   GEMM_NT_REG_STAGED, GEMM_NT_SB8, GEMM_NT_STRIP, GEMM_ORDER_GROUPED, GEMM_ORDER_PLAIN, GEMM_ORDER_ROW_MAJOR, GEMM_STORE_NT,
                   GEMM_STORE_PLAIN, GEMM_STORE_SC1, GEMM_TN_REG_TRANSPOSE, GEMM_TN_TR_FULL_ONLY, GEMM_TNG_PLAIN_ORDER, GEMM_TNG_PLAIN_PHASES)

_DT = {torch.float32: MTP_F32, torch.bfloat16: MTP_BF16}
def lib():
    return _lib.load()


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("mtp_amd ops take float32 / bfloat16 tensors, got %s" % t.dtype)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("mtp_amd ops run only on an MI355X device tensor (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("mtp_amd ops need contiguous tensors")
    # every launch goes to the current stream of the CURRENT device (_s): a tensor living on another GPU (a module moved with
    # .to('cuda:1') while cuda:0 is current, as multi-GPU runners do) would be dereferenced by the wrong device, unordered
    # against its own stream.  One process per GPU with torch.cuda.set_device(local_rank) is the supported setup.
    if t.device.index != torch.cuda.current_device():
        raise RuntimeError("mtp_amd ops: tensor on %s but the current device is cuda:%d -- call torch.cuda.set_device(%d) (or use "
                           "`with torch.cuda.device(...)`) before running the backbone" % (t.device, torch.cuda.current_device(), t.device.index))
    return t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _scratch(shape, device, dtype):
    """every workspace, partial buffer and self-allocated result of the wrappers below comes from here: plain torch.empty -- one seam, so the GPU tests can
    hand out guarded, poisoned buffers instead (a workspace overrun is seen; an element read before it is written turns the result into NaN)"""
    return torch.empty(shape, device=device, dtype=dtype)


def _f32(t):
    if t is not None and t.dtype != torch.float32:
        raise TypeError("expected a float32 tensor")
    return _p(t)


# ------------------------------------------------------------------------------------------------ GEMM
def _nt_args(a, w, out, epi, bias, bias_mod, res, res_mod, rowscale, rows_per_sample, aux, variant, n=None):
    M, K = a.shape
    N = w.shape[0] if n is None else n       # n: only the first n rows of w / columns of a wider `out` (row stride out.shape[1])
    assert w.shape[1] == K and out.shape[0] == M and out.shape[1] >= N and w.shape[0] >= N and a.dtype == w.dtype
    assert n is not None or out.shape[1] == N
    g = GemmArgs()
    g.A, g.B, g.C = _p(a), _p(w), _p(out)
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = K, K, out.shape[1]
    g.in_dtype, g.out_dtype, g.epilogue = _dt(a), _dt(out), epi
    g.bias, g.bias_mod = _f32(bias), bias_mod
    g.res, g.res_ld, g.res_mod = _f32(res), (res.shape[-1] if res is not None else 0), res_mod
    g.rowscale, g.rows_per_sample = _f32(rowscale), rows_per_sample
    g.aux, g.aux_ld = _p(aux), (aux.shape[-1] if aux is not None else 0)
    if aux is not None:
        assert aux.dtype == out.dtype and tuple(aux.shape) == (M, N) and out.shape[1] == N
    g.split_k, g.variant = 1, variant
    return g


def sampling_fwd_rider(x, w, b, avg, pooled, samp, B, Hp, Wp):
    """rvsa_sampling_fwd(...) as a rider of gemm_nt: the same arguments, the same results"""
    r = _lib.NtRider(kind=_lib.NT_RIDER_SAMPLING_FWD, act_dtype=_dt(x), x=_p(x), w=_f32(w), bias=_f32(b), avg=_f32(avg), pooled=_f32(pooled), samp=_f32(samp),
                     B=B, Hp=Hp, Wp=Wp, C=x.shape[-1], N=w.shape[0])
    return r


def sampling_bwd_win_rider(dsamp, w, avg, g):
    """rvsa_sampling_bwd_win(...) as a rider of gemm_nt"""
    r = _lib.NtRider(kind=_lib.NT_RIDER_SAMPLING_BWD_WIN, act_dtype=MTP_BF16, dsamp=_f32(dsamp), w=_f32(w), avg=_f32(avg), g=_f32(g),
                     windows=avg.shape[0], C=avg.shape[1], N=w.shape[0])
    return r


def gemm_nt(a, w, out, epi=EPI_BIAS, bias=None, bias_mod=0, res=None, res_mod=0, rowscale=None, rows_per_sample=0,
            aux=None, variant=0, n=None, rider=None):
    """out (M,N) = epilogue(a (M,K) @ w (N,K)^T).  rider (sampling_fwd_rider / sampling_bwd_win_rider): an independent small operator that runs inside the
    same launch on the CUs the GEMM leaves idle (mtp_gemm_nt_rider), or right behind the GEMM where the launch has none to lend."""
    g = _nt_args(a, w, out, epi, bias, bias_mod, res, res_mod, rowscale, rows_per_sample, aux, variant, n)
    if rider is not None:
        check(lib().mtp_gemm_nt_rider(C.byref(g), C.byref(rider), _s()), "mtp_gemm_nt_rider")
    else:
        check(lib().mtp_gemm_nt(C.byref(g), _s()), "mtp_gemm_nt")
    return out


def gemm_nt_rider_plan(a, w, out, rider, epi=EPI_BIAS, bias=None, bias_mod=0, res=None, res_mod=0, rowscale=None, rows_per_sample=0,
                       aux=None, variant=0, n=None, cus=0):
    """what gemm_nt(..., rider=rider) does on a stream of `cus` CUs (0: the device's; a CU-masked stream: the CUs of its mask), no launch: a
    _lib.NtRiderPlan (rides, gemm_wgs, riders, windows_per_rider, scratch_bytes, reason = NT_RIDE_*)"""
    g = _nt_args(a, w, out, epi, bias, bias_mod, res, res_mod, rowscale, rows_per_sample, aux, variant, n)
    plan = _lib.NtRiderPlan()
    check(lib().mtp_gemm_nt_rider_plan(C.byref(g), C.byref(rider), cus, C.byref(plan)), "mtp_gemm_nt_rider_plan")
    return plan


def gemm_nt_tile(a, w, out, epi=EPI_BIAS, bias=None, bias_mod=0, res=None, res_mod=0, rowscale=None, rows_per_sample=0,
                 aux=None, variant=0, n=None):
    """tile width (256 / 128; 64 = the strip kernel) of the kernel family gemm_nt(...) runs these arguments on (no launch)"""
    g = _nt_args(a, w, out, epi, bias, bias_mod, res, res_mod, rowscale, rows_per_sample, aux, variant, n)
    rc = lib().mtp_gemm_nt_tile(C.byref(g))
    if rc < 0:
        check(rc, "mtp_gemm_nt_tile")
    return rc


def gemm_nt_plan(a, w, out, epi=EPI_BIAS, bias=None, bias_mod=0, res=None, res_mod=0, rowscale=None, rows_per_sample=0,
                 aux=None, variant=0, n=None, cus=0):
    """the plan gemm_nt(...) follows for these arguments on a stream of `cus` CUs (0: the device's), no launch: a _lib.GemmNtPlan
    (family = GEMM_NT_FAMILY_*, tile_m, order, persistent, store_policy)"""
    g = _nt_args(a, w, out, epi, bias, bias_mod, res, res_mod, rowscale, rows_per_sample, aux, variant, n)
    plan = _lib.GemmNtPlan()
    check(lib().mtp_gemm_nt_plan(C.byref(g), cus, C.byref(plan)), "mtp_gemm_nt_plan")
    return plan


def pick_split_k(M, N, K):
    """enough (tile, split) work items for >= 2 resident workgroups on each of the 256 CUs"""
    # measured on MI355X (tools/probes/ab_tn.py): ~512 work items (2 per CU) is the sweet spot; odd splits are consistently slower
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    split = max(1, min(16, round(512 / tiles)))
    if split > 1 and split % 2:
        split += 1
    return max(1, min(split, K // 1024))


def effective_split_k(K, dtype, split):
    """the split launch_tn (csrc/gemm.hip) really runs: at most one K tile (64 bf16 / 32 f32 rows) per split, and no empty
    splits -- the number of partial tiles the workspace holds and a deferred reduction has to sum"""
    k_tiles = -(-K // (64 if dtype == torch.bfloat16 else 32))
    split = max(1, min(int(split), k_tiles))
    per = -(-k_tiles // split)
    return -(-k_tiles // per)


def gemm_tn(a, b, out, split_k=None, use_workspace=True, variant=0, colsum=None, defer=None, m=None):
    """out (M,N) f32 = a (K,M)^T @ b (K,N)   (weight gradient dW = dY^T X).
    colsum (M,) f32, optional: colsum += a.sum(0) -- the bias gradient, produced by the same pass over dY.
    m: use only the first m columns of a wider `a` (row stride a.shape[1])."""
    K, M = a.shape
    lda = M
    if m is not None:
        assert m <= M
        M = m
    N = b.shape[1]
    assert b.shape[0] == K and out.dtype == torch.float32 and out.numel() == M * N and a.dtype == b.dtype
    g = GemmArgs()
    if colsum is not None:
        assert colsum.dtype == torch.float32 and colsum.numel() == M and colsum.is_contiguous()
        g.colsum = _p(colsum)
    g.A, g.B, g.C = _p(a), _p(b), _p(out)
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = lda, N, N
    g.in_dtype, g.out_dtype, g.epilogue = _dt(a), MTP_F32, EPI_BIAS
    g.split_k = effective_split_k(K, a.dtype, pick_split_k(M, N, K) if split_k is None else split_k)
    g.variant = variant
    if g.split_k > 1 and use_workspace:
        ws = _scratch((g.split_k * M * N,), out.device, torch.float32)   # split-K partials (summed by the callee)
        g.aux = _p(ws)
        if defer is not None:     # ... or later, together with the other weight gradients of the block (sum_partials)
            g.defer_sum = 1
            defer.append((ws, out, M * N, g.split_k))
    check(lib().mtp_gemm_tn(C.byref(g), _s()), "mtp_gemm_tn")
    return out


MAX_GROUPED = 32      # MTP_MAX_GROUPED_GEMMS


def grouped_tiles(M, N):
    """256 x 256 output tiles (edge tiles included) of one problem in mtp_gemm_tn_grouped, or 0 when it cannot take the problem"""
    return -(-M // 256) * -(-N // 256) if M % 8 == 0 and N % 8 == 0 and M >= 8 and N >= 8 else 0


def grouped_splits(K, tiles):
    """pieces of the contraction for a problem of `tiles` output tiles: 1 unless the contraction is much longer than a transformer block's
    (InternImage's 192- / 384-channel levels: M, N <= 1536 over 131072 / 32768 tokens; the ViT FPN's second deconvolution: 64 tiles over
    4 x the tokens) -- then pieces of >= 4096 rows, at most enough of them for one round of the 256 CUs, each piece an own workgroup"""
    if K < 16384:
        return 1
    return max(1, min(64, K // 4096, 256 // tiles))


_low_streams = {}


def low_priority_stream(device):
    """a side stream of the device's lowest priority (mtp_stream_create_low_priority), wrapped for torch; one per device, kept for the process"""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _low_streams.get(idx)
    if st is None:
        h = C.c_void_p()
        with torch.cuda.device(idx):
            check(lib().mtp_stream_create_low_priority(C.byref(h)), "mtp_stream_create_low_priority")
        st = _low_streams[idx] = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))
    return st


_mask_streams = {}


def cu_mask_words(kind, part, parts=2, cus_per_xcc=32, xccs=8):
    """the CU bit mask (list of 32-bit words) of partition `part` of `parts`: bit i = XCC i % xccs, CU j = i // xccs of that XCC (gfx950, SPX mode).
    kind "interleaved": CU j belongs to partition j % parts (whole shader engines); "blocked": j * parts // cus_per_xcc (a slice of every engine).
    Every partition holds cus_per_xcc / parts CUs of EVERY XCC: the dispatcher hands each XCC every eighth workgroup whatever the mask says."""
    words = [0] * (cus_per_xcc * xccs // 32)
    for i in range(cus_per_xcc * xccs):
        j = i // xccs
        mine = (j % parts == part) if kind == "interleaved" else (j * parts // cus_per_xcc == part)
        if mine:
            words[i // 32] |= 1 << (i % 32)
    return words


def cu_mask_stream(device, words):
    """a stream restricted to the CUs of `words` (mtp_stream_create_cu_mask), wrapped for torch; one per (device, mask), kept for the process"""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, tuple(words))
    st = _mask_streams.get(key)
    if st is None:
        h = C.c_void_p()
        arr = (C.c_uint32 * len(words))(*words)
        with torch.cuda.device(idx):
            check(lib().mtp_stream_create_cu_mask(arr, len(words), C.byref(h)), "mtp_stream_create_cu_mask")
        st = _mask_streams[key] = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))
    return st


class WgradQueue:
    """Deferred weight gradients dW = dY^T X (+ bias gradient = column sums of dY): the weight gradients of a transformer block
    depend only on tensors the backward pass has anyway, so they are collected and launched together -- ONE
    mtp_gemm_tn_grouped launch whose 256 x 256 tiles fill the 256 CUs in whole rounds (4 ViT-L blocks = 768 tiles = 3 rounds),
    each tile with the full contraction: no split-K partials, no reduction launches.  Problems of a few tiles with a very long
    contraction are cut into pieces inside the same launch (grouped_splits; the kernel's own split_k + one reduction launch).  Problems
    the grouped kernel cannot take (f32 parity mode, sizes that are not multiples of 8 / 128) run immediately through gemm_tn."""

    def __init__(self, cus=256, variant=0, stream=None):
        self.jobs, self.tiles, self.cus, self.variant = [], 0, cus, variant
        # stream: launch on this (side) stream instead of the current one.  The weight gradients are off the backward pass's
        # critical path; next to the chain of data-gradient GEMMs (224 or 672 tiles on 256 CUs: 12.5 % of the CUs idle in the last
        # round) their tiles fill the idle CUs.  flush() orders the launch after everything issued so far; wait() orders the
        # current stream after the launches (call it before the gradients are consumed).
        self.stream, self.inflight = stream, []
        self.max_jobs = 0    # > 0: a burst goes out as soon as it holds this many problems (A/B of the burst size next to the side stream)
        self.launched = 0    # side-stream launches so far; launched - len(inflight) of them have been waited for by the current stream
        self.after = []      # callables run right after the launch (on its stream): e.g. copying a padded result into the gradient buffer
        # squared-norm by-product (round 6): with `sqn` (a 1-element f32 device tensor) every unsplit problem of a grouped launch also adds sum(dW^2) to it; `covered`
        # lists the gradient tensors whose norm has been accounted for that way (the clipping step sums the rest of the buffer only: FlatAdamW.step)
        self.sqn, self.covered = None, []

    def add(self, dy, x, dw, colsum=None, after=None, norm_of=None, norm_ok=True):
        """norm_of: the gradient tensor dw's values end up in when that is not dw itself (a re-laid copy made by `after`); norm_ok=False: `after` changes the values"""
        K, M = dy.shape
        N = x.shape[1]
        t = grouped_tiles(M, N)
        # the grouped kernel's own limits (gemm_tn_p8.hip: 32-bit DMA offsets -> K * ld * 2 < 4 GiB per operand; 16-byte aligned bases):
        # a problem outside them runs now through gemm_tn instead of failing the whole deferred launch several blocks later
        fits = (K * M * 2 < (1 << 32) and K * N * 2 < (1 << 32) and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and dw.data_ptr() % 16 == 0
                and dy.is_contiguous() and x.is_contiguous())
        if t == 0 or K % 128 or dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or not fits:
            gemm_tn(dy, x, dw, colsum=colsum)
            if after is not None:
                after()
            return False
        assert x.shape[0] == K and dw.dtype == torch.float32 and dw.numel() == M * N and dw.is_contiguous()
        splits = grouped_splits(K, t)
        part = _scratch((splits, M, N), dw.device, torch.float32) if splits > 1 else None
        use_sqn = self.sqn is not None and splits == 1 and norm_ok
        self.jobs.append((dy, x, dw, colsum, splits, part, use_sqn))     # (the references keep dY / X / the partial images alive until the launch)
        if use_sqn:
            self.covered.append(dw if norm_of is None else norm_of)
        if after is not None:
            self.after.append(after)
        self.tiles += t * splits
        return True

    def should_flush(self, next_tiles=0, next_jobs=4):
        """whole rounds of the CUs, or no room for another block's problems"""
        if not self.jobs:
            return False
        if len(self.jobs) + next_jobs > MAX_GROUPED or (self.max_jobs and len(self.jobs) >= self.max_jobs):
            return True
        rounds = -(-self.tiles // self.cus)
        return self.tiles / (rounds * self.cus) >= 0.93

    def flush(self):
        if self.stream is None or not self.jobs:
            return self._launch()
        ready = torch.cuda.Event()
        ready.record()
        held = list(self.jobs)           # dY / X / partial images stay referenced until the current stream has waited for the launch
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            self._launch()
            done = torch.cuda.Event()
            done.record()
        self.inflight.append((done, held))
        self.launched += 1

    def wait(self, keep=0):
        """the current stream waits for the side-stream launches, except the `keep` most recent ones"""
        while len(self.inflight) > keep:
            done, _ = self.inflight.pop(0)
            torch.cuda.current_stream().wait_event(done)

    def _launch(self):
        while self.jobs:
            chunk, self.jobs = self.jobs[:MAX_GROUPED], self.jobs[MAX_GROUPED:]
            arr = (GemmArgs * len(chunk))()
            for g, (dy, x, dw, cs, splits, part, use_sqn) in zip(arr, chunk):
                K, M = dy.shape
                N = x.shape[1]
                g.A, g.B, g.C = _p(dy), _p(x), _p(dw)
                g.M, g.N, g.K = M, N, K
                g.lda, g.ldb, g.ldc = M, N, N
                g.in_dtype, g.out_dtype, g.variant = MTP_BF16, MTP_F32, self.variant
                if splits > 1:
                    g.split_k, g.aux = splits, _p(part)
                if use_sqn:
                    g.workspace, g.workspace_bytes = _p(self.sqn), 4
                if cs is not None:
                    assert cs.dtype == torch.float32 and cs.numel() == M and cs.is_contiguous()
                    g.colsum = _p(cs)
            check(lib().mtp_gemm_tn_grouped(arr, len(chunk), _s()), "mtp_gemm_tn_grouped")
        after, self.after = self.after, []
        for fn in after:
            fn()
        self.tiles = 0


def sum_partials(jobs):
    """finish the deferred split-K reductions collected by gemm_tn(..., defer=jobs): one launch per 12 GEMMs"""
    while jobs:
        chunk, jobs[:] = jobs[:12], jobs[12:]
        n = len(chunk)
        P = C.c_void_p * n
        parts, outs = P(*[j[0].data_ptr() for j in chunk]), P(*[j[1].data_ptr() for j in chunk])
        numel, splits = (C.c_int64 * n)(*[j[2] for j in chunk]), (C.c_int * n)(*[j[3] for j in chunk])
        check(lib().mtp_sum_partials_batch(parts, outs, numel, splits, n, _s()), "mtp_sum_partials_batch")


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, y, mean=None, rstd=None, eps=1e-6, gelu=False):
    rows, Cc = x.shape
    check(lib().mtp_layernorm_fwd(_p(x), _dt(x), _f32(gamma), _f32(beta), _p(y), _dt(y), _f32(mean), _f32(rstd),
                                  rows, Cc, eps, int(gelu), _s()), "mtp_layernorm_fwd")
    return y


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, beta=None, gelu=False, dres=None, extra=None,
                  dx_copy=None, copy_scale=None, rows_per_sample=0, accumulate=False, defer=None, win_add=None, grid=None):
    """dx = [dres] + [extra] + LN'(dy); dgamma/dbeta (C,) f32 are overwritten (or accumulated into).  With `defer` (a list) the
    per-workgroup partials are kept and appended to it instead of being reduced: reduce_rows_deferred(defer) finishes several
    LayerNorms' parameter gradients in one launch."""
    rows, Cc = x.shape
    # (an in-kernel f32-atomic accumulation of dgamma / dbeta was measured: 512 workgroups hitting the same 2C addresses took
    #  the kernel from 61 to 106 us; per-workgroup partials + two 8 us reductions are faster)
    nblk = lib().mtp_layernorm_bwd_partial_rows(rows)
    part = _scratch((nblk, 2 * Cc), x.device, torch.float32)     # [dgamma partials | dbeta partials] per workgroup
    if win_add is not None:
        # dy_eff = dy + win_add[window(row)]: the RVSA sampling heads' input gradient, added per 7 x 7 window of the (B, Hp, Wp) token grid
        B, Hp, Wp = grid
        nh, nw = rvsa_windows(Hp, Wp)
        assert not gelu and tuple(win_add.shape) == (B * nh * nw, Cc) and B * Hp * Wp == rows
        check(lib().mtp_layernorm_bwd_win(_p(dy), _dt(dy), _p(x), _dt(x), _f32(mean), _f32(rstd), _f32(gamma), _f32(dres), _f32(extra), _p(dx), _dt(dx),
                                          _p(dx_copy), (_dt(dx_copy) if dx_copy is not None else 0), _f32(copy_scale), rows_per_sample,
                                          part.data_ptr(), part.data_ptr() + 4 * Cc, 2 * Cc, rows, Cc, _f32(win_add), B, Hp, Wp, _s()), "mtp_layernorm_bwd_win")
    else:
        check(lib().mtp_layernorm_bwd(_p(dy), _dt(dy), _p(x), _dt(x), _f32(mean), _f32(rstd), _f32(gamma), _f32(beta), int(gelu),
                                      _f32(dres), _f32(extra), _p(dx), _dt(dx), _p(dx_copy), (_dt(dx_copy) if dx_copy is not None else 0),
                                      _f32(copy_scale), rows_per_sample, part.data_ptr(), part.data_ptr() + 4 * Cc, 2 * Cc, rows, Cc, _s()),
              "mtp_layernorm_bwd")
    # weight and bias gradient adjacent in one buffer (the flat gradient buffer of mtp_amd.parallel) -> ONE reduction launch
    if defer is not None and _adjacent(dgamma, dbeta) and dgamma.numel() == Cc:
        defer.append((part, dgamma, accumulate))
    else:
        _reduce_pair(part, Cc, dgamma, dbeta, accumulate)
    return dx


def layernorm_residual_fwd(h, gamma, beta, x, layer_scale, out, out_act, mean, rstd, sample_scale=None, rows_per_sample=0, eps=1e-6):
    """out (f32) = x + sample_scale[row / rows_per_sample] * layer_scale * LayerNorm(h); out_act = its ACT copy (InternImage's post-norm residual)"""
    rows, Cc = h.shape
    check(lib().mtp_layernorm_residual_fwd(_p(h), _dt(h), _f32(gamma), _f32(beta), _f32(x), _f32(layer_scale), _f32(sample_scale), rows_per_sample,
                                           _f32(out), _p(out_act), _f32(mean), _f32(rstd), rows, Cc, eps, _s()), "mtp_layernorm_residual_fwd")
    return out


def layernorm_residual_bwd(dout, h, mean, rstd, gamma, beta, layer_scale, dh, dgamma, dbeta, dls, sample_scale=None, rows_per_sample=0, defer=None):
    """dh = LN'(s * layer_scale * dout); dgamma / dbeta / dls (C,) f32 ACCUMULATE the three parameter gradients (deferred with `defer`)"""
    rows, Cc = h.shape
    nblk = lib().mtp_layernorm_bwd_partial_rows(rows)
    part = _scratch((nblk, 3 * Cc), h.device, torch.float32)
    check(lib().mtp_layernorm_residual_bwd(_f32(dout), _p(h), _dt(h), _f32(mean), _f32(rstd), _f32(gamma), _f32(beta), _f32(layer_scale), _f32(sample_scale),
                                           rows_per_sample, _p(dh), part.data_ptr(), rows, Cc, _s()), "mtp_layernorm_residual_bwd")
    pair = _adjacent(dgamma, dbeta) and dgamma.numel() == Cc
    if defer is not None and pair:
        defer.append((part[:, :2 * Cc], dgamma, True))
        defer.append((part[:, 2 * Cc:], dls, True))
    else:
        _reduce_pair(part[:, :2 * Cc], Cc, dgamma, dbeta, True)
        reduce_rows(part[:, 2 * Cc:], dls, True)
    return dh


REDUCE_BATCH_MAX = 32


def reduce_rows_deferred(items):
    """items: (part (rows, cols) f32, out (first of `cols` contiguous floats), accumulate[, (R, C)]) tuples queued by layernorm_bwd(defer=...) /
    rvsa_attn_bwd(defer=...); equally-shaped ones go out together, <= REDUCE_BATCH_MAX per launch (mtp_reduce_rows_batched_f32; with (R, C) the
    transposed form mtp_reduce_rows_t_batched_f32: column a * C + b -> out[b * R + a]).  Empties the list."""
    groups = {}
    for it in items:
        part, out, acc = it[:3]
        tr = it[3] if len(it) > 3 else None
        groups.setdefault((tuple(part.shape), part.stride(0), bool(acc), tr), []).append((part, out))
    for ((rows, cols), ld, acc, tr), g in groups.items():
        for i0 in range(0, len(g), REDUCE_BATCH_MAX):
            chunk = g[i0:i0 + REDUCE_BATCH_MAX]
            n = len(chunk)
            P = C.c_void_p * n
            if tr is None:
                check(lib().mtp_reduce_rows_batched_f32(P(*[c[0].data_ptr() for c in chunk]), P(*[c[1].data_ptr() for c in chunk]), n, ld, rows, cols,
                                                        int(acc), _s()), "mtp_reduce_rows_batched_f32")
            else:
                check(lib().mtp_reduce_rows_t_batched_f32(P(*[c[0].data_ptr() for c in chunk]), P(*[c[1].data_ptr() for c in chunk]), n, ld, rows, tr[0], tr[1],
                                                          int(acc), _s()), "mtp_reduce_rows_t_batched_f32")
    del items[:]


def reduce_rows(part, out, accumulate=False):
    """out (+)= part.sum(0); part (rows, cols) f32, a column slice of a wider buffer is fine (row stride = part.stride(0))."""
    if not part.is_cuda:
        raise RuntimeError("mtp_amd ops run only on an MI355X device tensor (no CPU fallback)")
    assert part.dim() == 2 and part.stride(1) == 1 and part.dtype == torch.float32
    rows, cols = part.shape
    assert out.numel() == cols
    check(lib().mtp_reduce_rows_f32(part.data_ptr(), part.stride(0), _f32(out), rows, cols, int(accumulate), _s()), "mtp_reduce_rows_f32")
    return out


def _adjacent(a, b):
    """b starts right where a ends, in the same storage (true for consecutive parameters' gradients in the flat buffer)"""
    return (a.is_contiguous() and b.is_contiguous() and b.data_ptr() == a.data_ptr() + 4 * a.numel()
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


def _reduce_pair(part, n0, out0, out1, accumulate):
    """part (rows, n0 + n1) f32: column sums of [:, :n0] -> out0 and of [:, n0:] -> out1; one launch when out1 follows out0 in memory"""
    if _adjacent(out0, out1) and out0.numel() == n0:
        reduce_rows(part, out0.as_strided((part.shape[1],), (1,)), accumulate)
    else:
        reduce_rows(part[:, :n0], out0, accumulate)
        reduce_rows(part[:, n0:], out1, accumulate)


def copy_segments(srcs, dsts):
    """dsts[i].copy_(srcs[i]) for up to 12 contiguous f32 tensors in one launch."""
    n = len(srcs)
    assert n == len(dsts) and 0 < n <= 12
    for s, d in zip(srcs, dsts):
        assert s.dtype == d.dtype == torch.float32 and s.is_contiguous() and d.is_contiguous() and s.numel() == d.numel()
    P = C.c_void_p * n
    sp, dp = P(*[s.data_ptr() for s in srcs]), P(*[d.data_ptr() for d in dsts])
    cnt = (C.c_int64 * n)(*[s.numel() for s in srcs])
    check(lib().mtp_copy_segments_f32(sp, dp, cnt, n, _s()), "mtp_copy_segments_f32")


def colsum(dy, out, accumulate=False):
    M, N = dy.shape
    fn = lib().mtp_colsum_acc if accumulate else lib().mtp_colsum
    check(fn(_p(dy), _dt(dy), N, _f32(out), M, N, _s()), "mtp_colsum")
    return out


# ------------------------------------------------------------------------------------------------ layout
def patchify(img, cols, P=16):
    B, Cin, H, W = img.shape
    check(lib().mtp_patchify(_f32(img), _p(cols), _dt(cols), B, Cin, H, W, P, _s()), "mtp_patchify")
    return cols


def preprocess_patchify(img_u8, cols, P, mean, std, bgr_to_rgb=True, pad_divisor=32, pad_value=0.0):
    """uint8 (B,H,W,3) HWC image batch -> normalised patch rows `cols` (B*Hp*Wp, 3*P*P): MTP_DataPreprocessor's image
    path (channel flip, (x - mean) / std, pad to a multiple of pad_divisor) fused with the PatchEmbed im2col."""
    if not img_u8.is_cuda:
        raise RuntimeError("mtp_amd ops run only on an MI355X device tensor (no CPU fallback)")
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 4 and img_u8.shape[-1] == 3 and img_u8.is_contiguous()
    B, H, W, _ = img_u8.shape
    Hp, Wp = padded_grid(H, W, P, pad_divisor)
    assert tuple(cols.shape) == (B * Hp * Wp, 3 * P * P)
    m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    check(lib().mtp_preprocess_patchify(img_u8.data_ptr(), _p(cols), _dt(cols), B, H, W, P, pad_divisor, m3, s3, int(bool(bgr_to_rgb)),
                                        float(pad_value), _s()), "mtp_preprocess_patchify")
    return cols


def padded_grid(H, W, P, pad_divisor):
    """patch grid (Hp, Wp) of an H x W image padded bottom/right to a multiple of pad_divisor"""
    Hpad, Wpad = -(-H // pad_divisor) * pad_divisor, -(-W // pad_divisor) * pad_divisor
    assert Hpad % P == 0 and Wpad % P == 0
    return Hpad // P, Wpad // P


def unpatchify(cols, dimg, P=16):
    B, Cin, H, W = dimg.shape
    check(lib().mtp_unpatchify(_p(cols), _dt(cols), _f32(dimg), B, Cin, H, W, P, _s()), "mtp_unpatchify")
    return dimg


def cast(src, dst):
    assert src.numel() == dst.numel()
    check(lib().mtp_cast(_p(src), _dt(src), _p(dst), _dt(dst), src.numel(), _s()), "mtp_cast")
    return dst


def transpose_cast(src, dst):
    R, Cc = src.shape
    assert tuple(dst.shape) == (Cc, R)
    check(lib().mtp_transpose_cast(_f32(src), _p(dst), _dt(dst), R, Cc, _s()), "mtp_transpose_cast")
    return dst


def _wimg_table(rows, device):
    """rows (src_ptr, w, wt, R, C, f32_out, wd), one per matrix -> (the mtp_wimg_desc table in device memory, total_tiles, the images to keep alive);
    a matrix owns ceil(R / 64) * ceil(C / 64) consecutive tiles (= workgroups of the launch) from its tile0 on"""
    arr = (_lib.WimgDesc * len(rows))()
    tile0, keep = 0, []
    for i, (ptr, w, wt, R, Cc, f32_out, wd) in enumerate(rows):
        d = arr[i]
        d.src, d.w, d.wt = ptr, _p(w), _p(wt)
        d.R, d.C, d.tile0, d.f32_out, d.wd = R, Cc, tile0, int(bool(f32_out)), wd
        tile0 += ((R + 63) // 64) * ((Cc + 63) // 64)
        keep.append((w, wt))
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device), tile0, keep


class WeightImages:
    """Descriptor table (in device memory) for mtp_weight_images: every GEMM-side image of the f32 master weights is
    refreshed by ONE launch per optimizer step.  entries: (src (R,C) f32, w or None, wt or None, f32_out)."""

    def __init__(self, entries, act_dtype):
        rows = []
        for src, w, wt, f32_out in entries:
            assert src.dim() == 2 and src.dtype == torch.float32
            R, Cc = src.shape
            want = torch.float32 if f32_out else act_dtype
            for img in (w, wt):
                assert img is None or (img.dtype == want and img.numel() == R * Cc)
            rows.append((_f32(src), w, wt, R, Cc, f32_out, 0.0))
        self.table, self.total_tiles, self.keep = _wimg_table(rows, entries[0][0].device)
        self.n, self.act = len(rows), _DT[act_dtype]
        self.entries, self.act_dtype = list(entries), act_dtype       # (the entries keep the sources alive)

    def refresh(self):
        check(lib().mtp_weight_images(self.table.data_ptr(), self.n, self.total_tiles, self.act, _s()), "mtp_weight_images")


class AdamWImages:
    """Descriptor table for mtp_adamw_weight_images: ONE launch updates every parameter of the flat buffers (AdamW + gradient clipping, as adamw_flat) and writes the
    GEMM-side images of the parameters that have them from the same registers -- the separate image pass read each f32 master once more.
    flat: mtp_amd.parallel.FlatParams; wimg: the engine's WeightImages (its sources must be the flat parameters themselves); wd_of(name) -> weight decay.
    None is returned by build() when an image source is not a whole flat parameter (layer scale: the images are made from scaled temporaries)."""

    @staticmethod
    def build(flat, wimg, wd_of, lr_of=None):
        """lr_of(name) -> lr scale (layer-wise lr decay): step() then runs mtp_adamw_weight_images_lr with a per-descriptor scale table.  None: the plain entry point."""
        by_ptr = {}
        for src, w, wt, f32_out in (wimg.entries if wimg is not None else []):
            by_ptr[src.data_ptr()] = (src, w, wt, f32_out)
        base = flat.data.data_ptr()
        rows, scales = [], []
        used = 0
        for n in flat.names:
            if flat.groups[n] is None:
                continue
            off = flat.offsets[n]
            numel = 1
            for d in flat.shapes[n]:
                numel *= d
            ent = by_ptr.get(base + 4 * off)
            if ent is not None:
                src, w, wt, f32_out = ent
                if src.numel() != numel:
                    return None
                R, Cc = src.shape
                used += 1
            else:
                w = wt = None
                f32_out = False
                padded = (numel + 63) // 64 * 64          # FlatParams pads every parameter to 64 elements: the tail is zero and stays zero
                R, Cc = padded // 64, 64
            rows.append((base + 4 * off, w, wt, R, Cc, f32_out, float(wd_of(n))))
            scales.append(1.0 if lr_of is None else float(lr_of(n)))
        if used != len(by_ptr):
            return None               # an image whose source is not a flat parameter
        self = AdamWImages()
        self.table, self.total_tiles, self.keep = _wimg_table(rows, flat.data.device)
        self.n = len(rows)
        self.act = _DT[wimg.act_dtype] if wimg is not None else MTP_BF16
        self.lr = None if lr_of is None else torch.tensor(scales, dtype=torch.float32).to(flat.data.device)     # (one scale per descriptor)
        self.flat = flat
        return self

    def step(self, m, v, hyper, sqn, max_norm, grad_scale):
        f = self.flat
        fn, lr = ("mtp_adamw_weight_images", ()) if self.lr is None else ("mtp_adamw_weight_images_lr", (_f32(self.lr),))
        check(getattr(lib(), fn)(self.table.data_ptr(), *lr, self.n, self.total_tiles, self.act, _f32(f.data), _f32(f.grad), _f32(m), _f32(v), _f32(hyper),
                                 _f32(sqn), max_norm, grad_scale, _s()), fn)


def convt_pack(w, wg, wgT):
    Cin, Cout = w.shape[:2]
    dt = _dt(wg if wg is not None else wgT)
    check(lib().mtp_convt_pack(_f32(w), _p(wg), _p(wgT), dt, Cin, Cout, _s()), "mtp_convt_pack")


def convt_unpack_grad(dwg, dw):
    Cin, Cout = dw.shape[:2]
    check(lib().mtp_convt_unpack_grad(_f32(dwg), _f32(dw), Cin, Cout, _s()), "mtp_convt_unpack_grad")
    return dw


def tokens_to_nchw(x, out, B, Hp, Wp, levels):
    Cc = x.shape[-1]
    check(lib().mtp_tokens_to_nchw(_p(x), _dt(x), _p(out), _dt(out), B, Hp, Wp, Cc, levels, _s()), "mtp_tokens_to_nchw")
    return out


def nchw_to_tokens(f, out, B, Hp, Wp, levels):
    Cc = f.shape[1]
    check(lib().mtp_nchw_to_tokens(_p(f), _dt(f), _p(out), _dt(out), B, Hp, Wp, Cc, levels, _s()), "mtp_nchw_to_tokens")
    return out


def maxpool2_tokens_fwd(x, y, B, Hp, Wp):
    check(lib().mtp_maxpool2_tokens_fwd(_f32(x), _p(y), _dt(y), B, Hp, Wp, x.shape[-1], _s()), "mtp_maxpool2_tokens_fwd")
    return y


def maxpool2_tokens_bwd(x, dy, dx, B, Hp, Wp, accumulate=False):
    check(lib().mtp_maxpool2_tokens_bwd(_f32(x), _p(dy), _dt(dy), _f32(dx), int(accumulate), B, Hp, Wp, x.shape[-1], _s()), "mtp_maxpool2_tokens_bwd")
    return dx


def axpy(y, x, alpha=1.0):
    check(lib().mtp_axpy_f32(_f32(y), _f32(x), alpha, y.numel(), _s()), "mtp_axpy_f32")
    return y


def scale_rows_cast(src, dst, scale=None, rows_per_sample=0):
    rows, Cc = src.shape
    check(lib().mtp_scale_rows_cast(_f32(src), _p(dst), _dt(dst), _f32(scale), rows_per_sample, rows, Cc, _s()), "mtp_scale_rows_cast")
    return dst


# ------------------------------------------------------------------------------------------------ attention
def full_attn_fwd(qkv, o, lse, rel_h, rel_w, B, Hp, Wp, heads, scale):
    hd = qkv.shape[1] // (3 * heads)
    check(lib().mtp_full_attn_fwd(_p(qkv), _p(o), _f32(lse), _dt(qkv), _f32(rel_h), _f32(rel_w), B, Hp, Wp, heads, hd, scale, _s()), "mtp_full_attn_fwd")
    return o, lse


def full_attn_bwd(qkv, o, dout, lse, dqkv, rel_h, rel_w, drel_h, drel_w, B, Hp, Wp, heads, scale, accumulate=False, defer=None):
    hd = qkv.shape[1] // (3 * heads)
    rt = (2 * Hp - 1) + (2 * Wp - 1)
    part = _scratch((B * heads, rt * hd), qkv.device, torch.float32)
    nws = lib().mtp_full_attn_bwd_workspace_floats(B, Hp, Wp, heads)     # > 0 beyond 256 tokens (three-pass backward)
    ws = _scratch((nws,), qkv.device, torch.float32) if nws else None
    check(lib().mtp_full_attn_bwd(_p(qkv), _p(o), _p(dout), _f32(lse), _p(dqkv), _dt(qkv), _f32(rel_h), _f32(rel_w), _p(part), _p(ws),
                                  B, Hp, Wp, heads, hd, scale, _s()), "mtp_full_attn_bwd")
    if defer is not None and _adjacent(drel_h, drel_w) and drel_h.numel() == (2 * Hp - 1) * hd:
        defer.append((part, drel_h, accumulate))       # reduced with the burst's other partial rows (reduce_rows_deferred)
        return dqkv
    _reduce_pair(part, (2 * Hp - 1) * hd, drel_h, drel_w, accumulate)   # per-(image, head) partials -> the two parameters
    return dqkv


# kernel families, as include/mtp_hip.h names them (0 = none: the entry point would refuse the grid as unsupported)
# value 2 of the two full-attention tables is retired (it named the deleted "mfma1" family): never returned, never reused
FULL_FWD = {"v3": 1, "flash128": 3, "flash256": 4, "generic": 5}
FULL_BWD = {"v3": 1, "flash": 3, "three_pass": 4, "single_wg": 5}
RVSA_FWD = {"generic": 1, "mfma": 2}
RVSA_BWD = {"generic": 1, "mfma_dense": 2, "mfma_atomic": 3}


def full_attn_kernel(dtype, Hp, Wp, backward=False):
    """the kernel family full_attn_fwd / full_attn_bwd run for this dtype and grid (a FULL_FWD / FULL_BWD value, 0 = unsupported); no launch, no device"""
    rc = lib().mtp_full_attn_kernel(_DT[dtype], Hp, Wp, int(backward))
    if rc < 0:
        check(rc, "mtp_full_attn_kernel")
    return rc


def rvsa_attn_kernel(dtype, Hp, Wp, heads, backward=False):
    """the kernel family rvsa_attn_fwd / rvsa_attn_bwd run for this dtype and grid (a RVSA_FWD / RVSA_BWD value); no launch, no device"""
    rc = lib().mtp_rvsa_attn_kernel(_DT[dtype], Hp, Wp, heads, int(backward))
    if rc < 0:
        check(rc, "mtp_rvsa_attn_kernel")
    return rc


def rvsa_windows(Hp, Wp):
    """(nh, nw) windows of an RVSA block: must match RvsaWindows in csrc/common.h, the one C definition (the host sizes buffers with it before any call)"""
    nh = (Hp + (7 - Hp % 7) % 7) // 7
    nw = (Wp + (7 - Wp % 7) % 7) // 7
    return nh, nw


def rvsa_pool_fwd(x, avg, pooled, B, Hp, Wp):
    check(lib().mtp_rvsa_pool_fwd(_p(x), _dt(x), _f32(avg), _f32(pooled), B, Hp, Wp, x.shape[-1], _s()), "mtp_rvsa_pool_fwd")


def rvsa_pool_bwd(dpooled, avg, dx, B, Hp, Wp, accumulate=True):
    check(lib().mtp_rvsa_pool_bwd(_f32(dpooled), _f32(avg), _p(dx), _dt(dx), int(accumulate), B, Hp, Wp, dx.shape[-1], _s()), "mtp_rvsa_pool_bwd")


def rvsa_sampling_fwd(x, w, b, avg, pooled, samp, B, Hp, Wp):
    """pool -> LeakyReLU -> stacked 1x1 heads in one launch (mtp_rvsa_sampling_fwd)"""
    check(lib().mtp_rvsa_sampling_fwd(_p(x), _dt(x), _f32(w), _f32(b), _f32(avg), _f32(pooled), _f32(samp), B, Hp, Wp, x.shape[-1], w.shape[0], _s()),
          "mtp_rvsa_sampling_fwd")
    return samp


def rvsa_sampling_bwd(dsamp, w, avg, dx, B, Hp, Wp):
    """dx += broadcast((dsamp . w) * leaky'(avg) / 49) in one launch (mtp_rvsa_sampling_bwd)"""
    check(lib().mtp_rvsa_sampling_bwd(_f32(dsamp), _f32(w), _f32(avg), _p(dx), _dt(dx), B, Hp, Wp, dx.shape[-1], w.shape[0], _s()), "mtp_rvsa_sampling_bwd")
    return dx


def rvsa_sampling_bwd_win(dsamp, w, avg, g):
    """g (windows, C) f32 = (dsamp . w) * leaky'(avg) / 49 -- the per-window addend layernorm_bwd(win_add=...) spreads over the tokens"""
    R, Cc = avg.shape
    check(lib().mtp_rvsa_sampling_bwd_win(_f32(dsamp), _f32(w), _f32(avg), _f32(g), R, Cc, w.shape[0], _s()), "mtp_rvsa_sampling_bwd_win")
    return g


def small_linear_fwd(x, w, b, y):
    R, K = x.shape
    check(lib().mtp_small_linear_fwd(_f32(x), _f32(w), _f32(b), _f32(y), R, w.shape[0], K, _s()), "mtp_small_linear_fwd")
    return y


def small_linear_bwd(x, w, dy, dx, dw, db):
    """dx may be None (weight / bias gradients only)"""
    R, K = x.shape
    check(lib().mtp_small_linear_bwd(_f32(x), _f32(w), _f32(dy), _f32(dx), _f32(dw), _f32(db), R, w.shape[0], K, _s()), "mtp_small_linear_bwd")


def small_linear_dw_segments(x, dy, dws, dbs):
    """dws[j] (rows_j, K) += dy[:, rows of segment j]^T x, dbs[j] += column sums: the stacked heads' gradients straight into their parameters"""
    R, K = x.shape
    n = len(dws)
    assert 0 < n <= 4 and len(dbs) == n and sum(d.shape[0] for d in dws) == dy.shape[1]
    rows = (C.c_int64 * n)(*[d.shape[0] for d in dws])
    P = C.c_void_p * n
    check(lib().mtp_small_linear_dw_segments(_f32(x), _f32(dy), R, dy.shape[1], K, n, rows, P(*[_f32(d) for d in dws]), P(*[_f32(d) for d in dbs]), _s()),
          "mtp_small_linear_dw_segments")


SL_BATCH = 8


def small_linear_dw_segments_flush(jobs):
    """jobs: (x, dy, dws, dbs) tuples queued instead of small_linear_dw_segments calls (the stacked sampling heads of a burst of RVSA blocks):
    equally-shaped ones go out together, <= SL_BATCH per launch.  Empties the list."""
    groups = {}
    for x, dy, dws, dbs in jobs:
        groups.setdefault((tuple(x.shape), tuple(dy.shape), tuple(d.shape[0] for d in dws)), []).append((x, dy, dws, dbs))
    for ((R, K), (_, N), rows_), g in groups.items():
        nseg = len(rows_)
        rows = (C.c_int64 * nseg)(*rows_)
        for i0 in range(0, len(g), SL_BATCH):
            chunk = g[i0:i0 + SL_BATCH]
            n = len(chunk)
            P, PS = C.c_void_p * n, C.c_void_p * (n * nseg)
            check(lib().mtp_small_linear_dw_segments_batched(P(*[_f32(c[0]) for c in chunk]), P(*[_f32(c[1]) for c in chunk]), n, R, N, K, nseg, rows,
                                                             PS(*[_f32(d) for c in chunk for d in c[2]]), PS(*[_f32(d) for c in chunk for d in c[3]]), _s()),
                  "mtp_small_linear_dw_segments_batched")
    del jobs[:]


def rvsa_attn_fwd(qkv, samp, o, lse, rel_h, rel_w, table, B, Hp, Wp, heads, scale):
    hd = qkv.shape[1] // (3 * heads)
    check(lib().mtp_rvsa_attn_fwd(_p(qkv), _f32(samp), _p(o), _f32(lse), _dt(qkv), _f32(rel_h), _f32(rel_w), _f32(table),
                                  B, Hp, Wp, heads, hd, scale, _s()), "mtp_rvsa_attn_fwd")
    return o, lse


def rvsa_attn_bwd(qkv, samp, o, dout, lse, dqkv, dsamp, rel_h, rel_w, table, drel_h, drel_w, dtable, B, Hp, Wp, heads, scale, accumulate=False, defer=None):
    hd = qkv.shape[1] // (3 * heads)
    T, C3 = qkv.shape
    Cc = C3 // 3
    nh, nw = rvsa_windows(Hp, Wp)
    nblk = B * nh * nw * heads
    dev = qkv.device
    dkv = _scratch((T, 2 * Cc), dev, torch.float32)
    rel_part = _scratch((nblk, 26 * hd), dev, torch.float32)
    tab_part = _scratch((B * nh * nw, heads * 169), dev, torch.float32)     # (window, head, 169): contiguous per workgroup
    check(lib().mtp_rvsa_attn_bwd(_p(qkv), _f32(samp), _p(o), _p(dout), _f32(lse), _p(dqkv), _p(dkv), _f32(dsamp), _p(rel_part), _p(tab_part),
                                  _dt(qkv), _f32(rel_h), _f32(rel_w), _f32(table), B, Hp, Wp, heads, hd, scale, _s()), "mtp_rvsa_attn_bwd")
    if defer is not None and _adjacent(drel_h, drel_w) and drel_h.numel() == 13 * hd:
        # the partial rows wait for the burst's reduction launch (reduce_rows_deferred): one launch per burst of blocks instead of two per block
        defer.append((rel_part, drel_h, accumulate))
        defer.append((tab_part, dtable, accumulate, (heads, 169)))
        return dqkv
    _reduce_pair(rel_part, 13 * hd, drel_h, drel_w, accumulate)   # per-workgroup partials -> the parameters, no staging copies
    # per-(window, head) partials (heads, 169) -> the (169, heads) parameter gradient: one launch, transposed on the way
    check(lib().mtp_reduce_rows_t_f32(_p(tab_part), tab_part.shape[1], _f32(dtable), tab_part.shape[0], heads, 169, int(accumulate), _s()),
          "mtp_reduce_rows_t_f32")
    return dqkv


# ------------------------------------------------------------------------------------------------ optimizer
def zero_segments(base, start, count):
    """base[start[i] : start[i] + count[i]] = 0 for the int64 device tables start / count (one launch, one workgroup per entry)"""
    assert base.dtype == torch.float32 and start.dtype == torch.int64 and count.dtype == torch.int64 and start.numel() == count.numel()
    check(lib().mtp_zero_segments_f32(_p(base), start.data_ptr(), count.data_ptr(), start.numel(), _s()), "mtp_zero_segments_f32")


def sqnorm(g, out):
    check(lib().mtp_sqnorm_f32(_f32(g), _f32(out), g.numel(), _s()), "mtp_sqnorm_f32")
    return out


def sqnorm_segments(base, start, count, out):
    """out += sum(base[start[i] : start[i] + count[i]] ** 2) over the int64 device tables start / count (one launch)"""
    assert base.dtype == torch.float32 and start.dtype == torch.int64 and count.dtype == torch.int64 and start.numel() == count.numel()
    check(lib().mtp_sqnorm_segments_f32(_p(base), start.data_ptr(), count.data_ptr(), start.numel(), _f32(out), _s()), "mtp_sqnorm_segments_f32")
    return out


def adamw_flat(p, g, m, v, seg_start, seg_wd, hyper, sqn=None, max_norm=0.0, grad_scale=1.0):
    assert seg_start.dtype == torch.int64 and seg_start.is_cuda
    check(lib().mtp_adamw_flat(_f32(p), _f32(g), _f32(m), _f32(v), p.numel(), seg_start.data_ptr(), _f32(seg_wd), seg_start.numel(),
                               _f32(hyper), _f32(sqn), max_norm, grad_scale, _s()), "mtp_adamw_flat")


def adamw_flat_lr(p, g, m, v, seg_start, seg_wd, seg_lr, hyper, sqn=None, max_norm=0.0, grad_scale=1.0):
    """adamw_flat with layer-wise lr decay: segment s trains at lr = hyper[0] * seg_lr[s]"""
    assert seg_start.dtype == torch.int64 and seg_start.is_cuda and seg_lr.numel() == seg_start.numel() == seg_wd.numel()
    check(lib().mtp_adamw_flat_lr(_f32(p), _f32(g), _f32(m), _f32(v), p.numel(), seg_start.data_ptr(), _f32(seg_wd), _f32(seg_lr), seg_start.numel(),
                                  _f32(hyper), _f32(sqn), max_norm, grad_scale, _s()), "mtp_adamw_flat_lr")


# ------------------------------------------------------------------------------------------------ InternImage layers (csrc/conv.hip)
def pad8(n):
    return (n + 7) // 8 * 8


def conv_out(h, stride):
    return (h - 1) // stride + 1


def im2col3x3(x, strides, cols, N, H, W, Cin, stride):
    """x: any tensor addressed by element strides (sN, sH, sW, sC); cols (N*Ho*Wo, Kp) ACT"""
    Kp = cols.shape[1]
    assert cols.shape[0] == N * conv_out(H, stride) * conv_out(W, stride) and Kp >= 9 * Cin
    sN, sH, sW, sC = strides
    if not x.is_cuda:
        raise RuntimeError("mtp_amd ops run only on an MI355X device tensor (no CPU fallback)")
    check(lib().mtp_im2col3x3(x.data_ptr(), _dt(x), sN, sH, sW, sC, _p(cols), _dt(cols), N, H, W, Cin, stride, Kp, _s()), "mtp_im2col3x3")
    return cols


def col2im3x3(dcols, dx, strides, N, H, W, Cin, stride, accumulate=False):
    sN, sH, sW, sC = strides
    assert dx.dtype == torch.float32 and dx.is_cuda
    check(lib().mtp_col2im3x3(_p(dcols), _dt(dcols), dx.data_ptr(), sN, sH, sW, sC, N, H, W, Cin, stride, dcols.shape[1], int(accumulate), _s()), "mtp_col2im3x3")
    return dx


# kernel families of the operators below that have more than one kernel, as include/mtp_hip.h names them (MTP_CONV_KERNEL_*; 0 = the entry point
# would refuse the call as unsupported)
CONV_KERNEL = {"element": 1, "v8": 2, "p8": 3, "px4": 4}
_CONV_OP = {"im2col3x3": 0, "col2im3x3": 1, "dwconv3x3_fwd": 2, "dwconv3x3_bwd_dx": 3, "dwconv3x3_bwd_dw": 4}


def _ptr(t):
    return None if t is None else t.data_ptr()


def conv_kernel(op, src, dst, N, H, W, Cc, strides=(0, 0, 0, 0), stride=1, Kp=0, w=None, b=None):
    """the kernel `op` (a key of _CONV_OP) runs for these very tensors and sizes (a CONV_KERNEL value): the decision the entry point launches by; no launch,
    no device.  src / dst: the operator's source and destination (im2col3x3: x, cols; col2im3x3: dcols, dx; dwconv3x3_fwd: x, y; _bwd_dx: dy, dx;
    _bwd_dw: dy, the partials or None = the wrapper's own 16-byte aligned workspace); Cc = Cin for the two gathers"""
    dptr = 16 if (dst is None and op == "dwconv3x3_bwd_dw") else _ptr(dst)
    sN, sH, sW, sC = strides
    rc = lib().mtp_conv_kernel(_CONV_OP[op], _ptr(src), _dt(src), sN, sH, sW, sC, dptr, _dt(dst) if dst is not None else 0, _ptr(w), _ptr(b), N, H, W, Cc, stride, Kp)
    if rc < 0:
        check(rc, "mtp_conv_kernel")
    return rc


def conv3x3_pack(w, w2, w2t):
    Cout, Cin = w.shape[:2]
    img = w2 if w2 is not None else w2t
    Kp = w2.shape[1] if w2 is not None else w2t.shape[0]
    check(lib().mtp_conv3x3_pack(_f32(w), _p(w2), _p(w2t), _dt(img), Cout, Cin, Kp, _s()), "mtp_conv3x3_pack")


def conv3x3_unpack_grad(dw2, dw):
    Cout, Cin = dw.shape[:2]
    check(lib().mtp_conv3x3_unpack_grad(_f32(dw2), _f32(dw), Cout, Cin, dw2.shape[1], _s()), "mtp_conv3x3_unpack_grad")
    return dw


def pack_rows_padded(w, wp, wpt):
    R, Cc = w.shape
    img = wp if wp is not None else wpt
    Rp = wp.shape[0] if wp is not None else wpt.shape[1]
    check(lib().mtp_pack_rows_padded(_f32(w), _p(wp), _p(wpt), _dt(img), R, Cc, Rp, _s()), "mtp_pack_rows_padded")


def dwconv3x3_fwd(x, w, b, y, N, H, W):
    check(lib().mtp_dwconv3x3_fwd(_p(x), _f32(w), _f32(b), _p(y), _dt(x), N, H, W, x.shape[-1], _s()), "mtp_dwconv3x3_fwd")
    return y


def dwconv3x3_bwd_dx(dy, w, dx, N, H, W, accumulate=False):
    check(lib().mtp_dwconv3x3_bwd_dx(_p(dy), _dt(dy), _f32(w), _f32(dx), int(accumulate), N, H, W, dy.shape[-1], _s()), "mtp_dwconv3x3_bwd_dx")
    return dx


def dwconv3x3_bwd_dw(dy, x, dw, db, N, H, W, accumulate=False):
    """dw (C,1,3,3) f32, db (C,) f32"""
    Cc = dy.shape[-1]
    nb = lib().mtp_dwconv3x3_bwd_dw_partial_rows(N, H, W)
    part = _scratch((nb, 10 * Cc), dy.device, torch.float32)
    check(lib().mtp_dwconv3x3_bwd_dw(_p(dy), _p(x), _dt(dy), _p(part), N, H, W, Cc, _s()), "mtp_dwconv3x3_bwd_dw")
    _reduce_pair(part, 9 * Cc, dw, db, accumulate)


def dwconv_fwd(x, w, b, y, N, H, W, k):
    """depth-wise k x k (any odd k; InternImage-H/G's dw_kernel_size): w (C, 1, k, k) f32"""
    check(lib().mtp_dwconv_fwd(_p(x), _f32(w), _f32(b), _p(y), _dt(x), N, H, W, x.shape[-1], int(k), _s()), "mtp_dwconv_fwd")
    return y


def dwconv_bwd_dx(dy, w, dx, N, H, W, k, accumulate=False):
    check(lib().mtp_dwconv_bwd_dx(_p(dy), _dt(dy), _f32(w), _f32(dx), int(accumulate), N, H, W, dy.shape[-1], int(k), _s()), "mtp_dwconv_bwd_dx")
    return dx


def dwconv_bwd_dw(dy, x, dw, db, N, H, W, k):
    """dw (C, 1, k, k) / db (C,) f32 += the weight / bias gradient (f32 atomics: accumulates)"""
    check(lib().mtp_dwconv_bwd_dw(_p(dy), _p(x), _dt(dy), _f32(dw), _f32(db), N, H, W, dy.shape[-1], int(k), _s()), "mtp_dwconv_bwd_dw")


def center_feature_scale_fwd(y, xp, logits, out, G):
    rows, Cc = y.shape
    check(lib().mtp_center_feature_scale_fwd(_p(y), _p(xp), _p(logits), logits.shape[1], _p(out), _dt(y), rows, G, Cc // G, _s()), "mtp_center_feature_scale_fwd")
    return out


def center_feature_scale_bwd(dout, y, xp, logits, dy, dxp, dlogits, G):
    rows, Cc = y.shape
    assert dlogits.shape == logits.shape
    check(lib().mtp_center_feature_scale_bwd(_p(dout), _p(y), _p(xp), _p(logits), logits.shape[1], _p(dy), _f32(dxp), _p(dlogits), _dt(y), rows, G, Cc // G, _s()),
          "mtp_center_feature_scale_bwd")
    return dy


def softmax_groups_fwd(logits, prob, G, P):
    rows = logits.shape[0]
    check(lib().mtp_softmax_groups_fwd(_p(logits), logits.shape[1], _p(prob), _dt(logits), rows, G, P, _s()), "mtp_softmax_groups_fwd")
    return prob


def softmax_groups_bwd(prob, dprob, dlogits, G, P):
    rows = dlogits.shape[0]
    check(lib().mtp_softmax_groups_bwd(_p(prob), _f32(dprob), _p(dlogits), dlogits.shape[1], _dt(prob), rows, G, P, _s()), "mtp_softmax_groups_bwd")
    return dlogits


def scale_residual_fwd(x, z, gamma, out, out_act=None, sample_scale=None, rows_per_sample=0):
    rows, Cc = x.shape
    check(lib().mtp_scale_residual_fwd(_f32(x), _p(z), _dt(z), _f32(gamma), _f32(sample_scale), rows_per_sample, _f32(out), _p(out_act), rows, Cc, _s()),
          "mtp_scale_residual_fwd")
    return out


def scale_residual_bwd(dout, z, gamma, dz, dgamma, sample_scale=None, rows_per_sample=0, accumulate=False):
    rows, Cc = dout.shape
    nb = lib().mtp_scale_residual_bwd_partial_rows(rows)
    part = _scratch((nb, Cc), dout.device, torch.float32)
    check(lib().mtp_scale_residual_bwd(_f32(dout), _p(z), _dt(z), _f32(gamma), _f32(sample_scale), rows_per_sample, _p(dz), _p(part), rows, Cc, _s()),
          "mtp_scale_residual_bwd")
    reduce_rows(part, dgamma, accumulate)
    return dz


def cast_pad_rows(src, dst):
    """src (rows, n) f32 -> dst (rows, ld >= n) ACT, columns n .. ld zero"""
    rows, n = src.shape
    assert dst.shape[0] == rows and dst.shape[1] >= n
    check(lib().mtp_cast_pad_rows(_f32(src), n, _p(dst), _dt(dst), dst.shape[1], rows, _s()), "mtp_cast_pad_rows")
    return dst


def copy_rows(src, dst, n):
    """dst[:, :n] = src[:, :n] (same dtype, 2-D contiguous buffers of different widths)"""
    assert src.dtype == dst.dtype and src.shape[0] == dst.shape[0]
    check(lib().mtp_copy_rows(_p(src), src.shape[1], _p(dst), dst.shape[1], _dt(src), n, src.shape[0], _s()), "mtp_copy_rows")
    return dst


# ------------------------------------------------------------------------------------------------ UperNet decode head (csrc/decode_head.hip)
def _ld(t):
    """row pitch of a 2-D row-major tensor or of a column slice of one"""
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


def _pv(t):
    """device pointer of a (possibly column-sliced) 2-D map"""
    if not t.is_cuda:
        raise RuntimeError("mtp_amd ops run only on an MI355X device tensor (no CPU fallback)")
    assert t.stride(-1) == 1
    return t.data_ptr()


def bn_sums(x, center=None):
    """x (rows, C) ACT (a column slice is fine) -> (2C,) f32 [sum (x - center) | sum (x - center)^2] (center (C,) f32 or None = 0), summed in a fixed
    order (bit-identical across runs)"""
    rows, Cc = x.shape
    part = _scratch((lib().mtp_bn_partial_rows(rows), 2 * Cc), x.device, torch.float32)
    sums = _scratch((2 * Cc,), x.device, torch.float32)
    check(lib().mtp_bn_stats(_pv(x), _dt(x), _ld(x), _f32(center), _p(part), _p(sums), rows, Cc, _s()), "mtp_bn_stats")
    return sums


def bn_finalize(sums, count, running_mean, running_var, mean, rstd, momentum=0.1, eps=1e-5, center=None):
    """sums None: the eval statistics from the running ones; center: what bn_sums(x, center) was centred on"""
    check(lib().mtp_bn_finalize(_f32(sums), _f32(center), float(count), _f32(running_mean), _f32(running_var), momentum, eps, _f32(mean), _f32(rstd), mean.numel(), _s()),
          "mtp_bn_finalize")


def bn_apply(x, mean, rstd, gamma, beta, y, relu=True):
    rows, Cc = x.shape
    assert y.shape == x.shape
    check(lib().mtp_bn_apply(_pv(x), _dt(x), _ld(x), _f32(mean), _f32(rstd), _f32(gamma), _f32(beta), int(relu), _pv(y), _dt(y), _ld(y), rows, Cc, _s()),
          "mtp_bn_apply")
    return y


def bn_bwd_sums(dy, x, mean, rstd, gamma, beta, relu=True):
    """(2C,) f32 [sum dy' | sum dy' xhat] = [d beta | d gamma] of this batch"""
    rows, Cc = x.shape
    part = _scratch((lib().mtp_bn_partial_rows(rows), 2 * Cc), x.device, torch.float32)
    sums = _scratch((2 * Cc,), x.device, torch.float32)
    check(lib().mtp_bn_bwd_stats(_pv(dy), _dt(dy), _ld(dy), _pv(x), _dt(x), _ld(x), _f32(mean), _f32(rstd), _f32(gamma), _f32(beta), int(relu), _p(part),
                                 _p(sums), rows, Cc, _s()), "mtp_bn_bwd_stats")
    return sums


def bn_bwd_dx(dy, x, mean, rstd, gamma, beta, sums, count, dx, relu=True):
    rows, Cc = x.shape
    check(lib().mtp_bn_bwd_dx(_pv(dy), _dt(dy), _ld(dy), _pv(x), _dt(x), _ld(x), _f32(mean), _f32(rstd), _f32(gamma), _f32(beta), int(relu), _f32(sums),
                              float(count), _pv(dx), _dt(dx), _ld(dx), rows, Cc, _s()), "mtp_bn_bwd_dx")
    return dx


def resize_bilinear_fwd(x, y, N, Hi, Wi, Ho, Wo, accumulate=False):
    """x (N*Hi*Wi, C), y (N*Ho*Wo, C) channels-last (column slices allowed); align_corners=False"""
    Cc = x.shape[1]
    assert y.shape[1] == Cc and x.shape[0] == N * Hi * Wi and y.shape[0] == N * Ho * Wo
    check(lib().mtp_resize_bilinear_fwd(_pv(x), _dt(x), _ld(x), _pv(y), _dt(y), _ld(y), N, Hi, Wi, Ho, Wo, Cc, int(accumulate), _s()),
          "mtp_resize_bilinear_fwd")
    return y


def resize_bilinear_bwd(dy, dx, N, Hi, Wi, Ho, Wo, accumulate=False):
    """dx (N*Hi*Wi, C) f32 (=/+=) from dy (N*Ho*Wo, C)"""
    Cc = dx.shape[1]
    assert dx.dtype == torch.float32 and dy.shape[1] == Cc and dx.shape[0] == N * Hi * Wi and dy.shape[0] == N * Ho * Wo
    check(lib().mtp_resize_bilinear_bwd(_pv(dy), _dt(dy), _ld(dy), _pv(dx), _ld(dx), N, Hi, Wi, Ho, Wo, Cc, int(accumulate), _s()), "mtp_resize_bilinear_bwd")
    return dx


def adaptive_avg_pool_fwd(x, y, N, H, W, S):
    Cc = x.shape[1]
    assert y.shape == (N * S * S, Cc)
    check(lib().mtp_adaptive_avg_pool_fwd(_pv(x), _dt(x), _ld(x), _p(y), _dt(y), N, H, W, Cc, S, _s()), "mtp_adaptive_avg_pool_fwd")
    return y


def adaptive_avg_pool_bwd(dy, dx, N, H, W, S, accumulate=False):
    Cc = dx.shape[1]
    assert dx.dtype == torch.float32 and dy.shape == (N * S * S, Cc)
    check(lib().mtp_adaptive_avg_pool_bwd(_p(dy), _dt(dy), _pv(dx), _ld(dx), N, H, W, Cc, S, int(accumulate), _s()), "mtp_adaptive_avg_pool_bwd")
    return dx


def channel_scale(x, mask, rows_per_sample, y):
    """Dropout2d with an explicit (N, C) f32 mask of 0 and 1 / (1 - p)"""
    rows, Cc = x.shape
    assert mask.shape[1] == Cc and y.shape == x.shape
    check(lib().mtp_channel_scale(_pv(x), _dt(x), _ld(x), _f32(mask), rows_per_sample, _pv(y), _dt(y), _ld(y), rows, Cc, _s()), "mtp_channel_scale")
    return y


def seg_ce(logits, K, N, h, w, labels, ignore_index=255, loss_weight=1.0):
    """logits (N*h*w, ld >= K) ACT, labels (N, H, W) uint8 / int64 -> (loss () f32, dlogits (N*h*w, ld) f32, columns K .. ld zero)"""
    assert labels.dim() == 3 and labels.dtype in (torch.uint8, torch.int64) and labels.is_contiguous() and labels.shape[0] == N
    H, W = labels.shape[1:]
    ld = logits.shape[1]
    bad = ((labels != ignore_index) & (labels.long() >= K)).any()        # (uint8 / int64 labels: only the upper bound can fail for uint8)
    if labels.dtype == torch.int64:
        bad = bad | ((labels != ignore_index) & (labels < 0)).any()
    if bool(bad):
        raise ValueError("seg_ce: labels outside [0, %d) that are not ignore_index (%d)" % (K, ignore_index))
    ws = _scratch(((lib().mtp_seg_ce_workspace_bytes(N, H, W, K) + 3) // 4,), logits.device, torch.float32)
    loss = _scratch((), logits.device, torch.float32)
    dlogits = _scratch((logits.shape[0], ld), logits.device, torch.float32).zero_() if ld != K else \
        _scratch((logits.shape[0], ld), logits.device, torch.float32)
    check(lib().mtp_seg_ce(_p(logits), _dt(logits), ld, N, h, w, K, _p(labels), labels.element_size(), H, W, int(ignore_index), float(loss_weight), _p(loss),
                           _p(dlogits), ld, _p(ws), ws.numel() * 4, _s()), "mtp_seg_ce")
    return loss, dlogits


# ------------------------------------------------------------------------------------------------ change detection (csrc/unet_head.hip)
FUSE_POLICIES = {"concat": _lib.FUSE_CONCAT, "sum": _lib.FUSE_SUM, "diff": _lib.FUSE_DIFF, "abs_diff": _lib.FUSE_ABS_DIFF}


def fuse_policy(policy):
    try:
        return FUSE_POLICIES[policy]
    except (KeyError, TypeError):
        raise ValueError("unknown fusion policy %r (one of %s)" % (policy, ", ".join(sorted(FUSE_POLICIES))))


def fuse_pair_fwd(f, out, policy):
    """f (2N, C, H, W) NCHW f32 / bf16, 'from' samples first -> out (N*H*W, C -- 2C for 'concat') channels-last (a column slice is fine)"""
    B, Cc, H, W = f.shape
    N = B // 2
    assert B == 2 * N and out.shape == (N * H * W, 2 * Cc if policy == "concat" else Cc)
    check(lib().mtp_fuse_pair_fwd(_p(f), _dt(f), _pv(out), _dt(out), _ld(out), N, Cc, H, W, fuse_policy(policy), _s()), "mtp_fuse_pair_fwd")
    return out


def fuse_pair_bwd(g, f, df, policy):
    """g (N*H*W, C | 2C) f32 (a column slice is fine), f the forward's input (read for 'abs_diff' only) -> df (2N, C, H, W) f32, both halves"""
    B, Cc, H, W = df.shape
    N = B // 2
    assert B == 2 * N and df.dtype == torch.float32 and g.shape == (N * H * W, 2 * Cc if policy == "concat" else Cc)
    assert f is None or f.shape == df.shape
    pol = fuse_policy(policy)
    fin = f if policy == "abs_diff" else None
    assert g.dtype == torch.float32
    check(lib().mtp_fuse_pair_bwd(_pv(g), _ld(g), _p(fin), _dt(fin) if fin is not None else 0, _f32(df), N, Cc, H, W, pol, _s()), "mtp_fuse_pair_bwd")
    return df


def unet_up_cat_fwd(x, skip, y, N, h, w, hs=0, ws=0):
    """y (N*2h*2w, Cx + Cs) = [x (N*h*w, Cx) nearest x2 | skip (N*hs*ws, Cs) resized bilinearly to 2h x 2w]; skip None: the skip-less block.
    Column slices allowed everywhere."""
    Cx = x.shape[1]
    Cs = 0 if skip is None else skip.shape[1]
    assert x.shape[0] == N * h * w and y.shape == (4 * N * h * w, Cx + Cs) and (skip is None or (skip.dtype == x.dtype and skip.shape[0] == N * hs * ws))
    check(lib().mtp_unet_up_cat_fwd(_pv(x), _ld(x), Cx, None if skip is None else _pv(skip), 0 if skip is None else _ld(skip), Cs, _dt(x), _pv(y), _dt(y),
                                    _ld(y), N, h, w, hs, ws, _s()), "mtp_unet_up_cat_fwd")
    return y


def unet_up_cat_bwd(dy, dx, dskip, N, h, w, hs=0, ws=0, accumulate=False):
    """dy (N*2h*2w, Cx + Cs) f32 -> dx (N*h*w, Cx) f32 and dskip (N*hs*ws, Cs) f32 (None: no skip), = / += (accumulate)"""
    Cx = dx.shape[1]
    Cs = 0 if dskip is None else dskip.shape[1]
    assert dy.dtype == dx.dtype == torch.float32 and dx.shape[0] == N * h * w and dy.shape == (4 * N * h * w, Cx + Cs)
    assert dskip is None or (dskip.dtype == torch.float32 and dskip.shape[0] == N * hs * ws)
    check(lib().mtp_unet_up_cat_bwd(_pv(dy), _ld(dy), _pv(dx), _ld(dx), Cx, None if dskip is None else _pv(dskip), 0 if dskip is None else _ld(dskip), Cs,
                                    N, h, w, hs, ws, int(accumulate), _s()), "mtp_unet_up_cat_bwd")
    return dx, dskip


# ------------------------------------------------------------------------------------------------ segmentation evaluation (csrc/seg_eval.hip)
SEG_MAX_CLASSES = 256      # the arg-max / area kernels keep 3 x K counters per workgroup in LDS


def _acc_pitch(acc, K):
    """pixel pitch of an accumulator (N, H, W, C >= K rounded up to 4) f32: contiguous, or the leading columns of a wider contiguous map"""
    assert acc.dim() == 4 and acc.dtype == torch.float32 and acc.stride(3) == 1 and acc.shape[3] >= (K + 3) // 4 * 4
    lda = acc.stride(2)
    assert lda >= acc.shape[3] and acc.stride(1) == acc.shape[2] * lda and acc.stride(0) == acc.shape[1] * acc.shape[2] * lda
    return lda


def _check_classes(name, t, K, ignore_index=None):
    """every value in [0, K) (or ignore_index): the kernels index LDS counters with them"""
    if t.dtype not in (torch.uint8, torch.int64) or not t.is_contiguous():
        raise TypeError("%s must be a contiguous uint8 / int64 tensor" % name)
    keep = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else (t != ignore_index)
    bad = (keep & (t.long() >= K)).any()         # (uint8: only the upper bound can fail)
    if t.dtype == torch.int64:
        bad = bad | (keep & (t < 0)).any()
    if bool(bad):
        raise ValueError("%s outside [0, %d)%s" % (name, K, "" if ignore_index is None else " that are not ignore_index (%d)" % ignore_index))


def _check_areas(areas, K):
    if K > SEG_MAX_CLASSES:
        raise ValueError("at most %d classes (got %d)" % (SEG_MAX_CLASSES, K))
    assert areas.dtype == torch.int64 and areas.shape == (3, K) and areas.is_contiguous()


def seg_window_accumulate(logits, K, N, h, w, acc, y1, x1, Hc, Wc):
    """acc[:, y1:y1 + Hc, x1:x1 + Wc, :K] += bilinear resize of logits (N*h*w, ld >= K rounded up to 4) ACT to (Hc, Wc); acc (N, H, W, >= K) f32"""
    lda = _acc_pitch(acc, K)
    assert logits.shape[0] == N * h * w and acc.shape[0] == N
    H, W = acc.shape[1:3]
    if y1 < 0 or x1 < 0 or y1 + Hc > H or x1 + Wc > W:
        raise ValueError("window (%d, %d) + (%d, %d) outside the %d x %d map" % (y1, x1, Hc, Wc, H, W))
    check(lib().mtp_seg_window_accumulate(_pv(logits), _dt(logits), _ld(logits), N, h, w, K, _pv(acc), lda, H, W, y1, x1, Hc, Wc, _s()),
          "mtp_seg_window_accumulate")
    return acc


def seg_argmax_areas(acc, K, cy=None, cx=None, pred=None, seg_logits=None, labels=None, areas=None, ignore_index=255, write_back=False):
    """one pass over acc (N, H, W, >= K) f32: / (cy[y] * cx[x]) (int32 window counts; None = 1), arg-max over the first K columns -> pred (N, H, W) uint8,
    the divided values -> seg_logits (N, K, H, W) f32 and / or back into acc (write_back); with labels (N, H, W) uint8 / int64 and areas (3, K) int64:
    areas += (intersect, pred, label) histograms over the pixels whose label is not ignore_index.  Any output may be None."""
    if K > SEG_MAX_CLASSES:
        raise ValueError("at most %d classes (got %d)" % (SEG_MAX_CLASSES, K))
    lda = _acc_pitch(acc, K)
    N, H, W = acc.shape[:3]
    if (cy is None) != (cx is None) or (labels is None) != (areas is None):
        raise ValueError("cy and cx, labels and areas go together")
    if cy is not None:
        assert cy.dtype == torch.int32 and cx.dtype == torch.int32 and cy.shape == (H,) and cx.shape == (W,)
    if pred is not None:
        assert pred.dtype == torch.uint8 and pred.shape == (N, H, W)
    if seg_logits is not None:
        assert seg_logits.dtype == torch.float32 and seg_logits.shape == (N, K, H, W)
    if labels is not None:
        assert labels.shape == (N, H, W)
        _check_classes("labels", labels, K, ignore_index)
        _check_areas(areas, K)
    check(lib().mtp_seg_argmax_areas(_pv(acc), lda, N, H, W, K, _p(cy), _p(cx), int(write_back), _p(pred), _p(seg_logits), _p(labels),
                                     0 if labels is None else labels.element_size(), int(ignore_index), _p(areas), _s()), "mtp_seg_argmax_areas")
    return pred


def seg_areas(pred, labels, K, areas, ignore_index=255):
    """areas (3, K) int64 += (intersect, pred, label) histograms of an existing prediction; pred / labels: same shape, uint8 or int64"""
    _check_areas(areas, K)
    if pred.shape != labels.shape:
        raise ValueError("pred %s and labels %s differ in shape" % (tuple(pred.shape), tuple(labels.shape)))
    _check_classes("pred", pred, K)
    _check_classes("labels", labels, K, ignore_index)
    check(lib().mtp_seg_areas(_p(pred), pred.element_size(), _p(labels), labels.element_size(), pred.numel(), K, int(ignore_index), _p(areas), _s()),
          "mtp_seg_areas")
    return areas


# ------------------------------------------------------------------------------------------------ scene classification (csrc/cls_head.hip)
CLS_MAX_TOPK = 8           # mtp_cls_hits takes its k list by value
_CLS_OUTPUTS = ("logits", "prob", "pred", "loss_rows", "loss", "dlogits")
_cls_counters = {}


def _cls_counter(device):
    """the arrival counter of mtp_cls_ce: one zeroed uint32 per (device, stream), which the kernel leaves at zero -- not from _scratch (no fill launch)"""
    key = (device.index, _s())
    c = _cls_counters.get(key)
    if c is None:
        c = _cls_counters[key] = torch.zeros(4, device=device, dtype=torch.int32)
    return c


def _check_labels(name, labels, N, K):
    if labels.dtype != torch.int64 or labels.shape != (N,) or not labels.is_contiguous():
        raise TypeError("%s: labels must be a contiguous int64 tensor of shape (%d,)" % (name, N))
    if bool(((labels < 0) | (labels >= K)).any()):
        raise ValueError("%s: labels outside [0, %d)" % (name, K))


def gap_fwd(x, pooled=None):
    """x (N, C, ...) contiguous f32 / bf16 -> pooled (N, C) f32, the mean over the trailing dimensions"""
    assert x.dim() >= 3
    N, Cc = x.shape[:2]
    HW = x[0, 0].numel()
    pooled = _scratch((N, Cc), x.device, torch.float32) if pooled is None else pooled
    assert pooled.shape == (N, Cc)
    check(lib().mtp_gap_fwd(_p(x), _dt(x), _f32(pooled), N, Cc, HW, _s()), "mtp_gap_fwd")
    return pooled


def gap_bwd(dpooled, dx):
    """dx (N, C, ...) f32 / bf16 = dpooled (N, C) f32 / HW broadcast; every element of dx is overwritten"""
    N, Cc = dx.shape[:2]
    assert dpooled.shape == (N, Cc)
    check(lib().mtp_gap_bwd(_f32(dpooled), _p(dx), _dt(dx), N, Cc, dx[0, 0].numel(), _s()), "mtp_gap_bwd")
    return dx


def cls_ce(pooled, w, b, labels=None, loss_weight=1.0, outputs=None, check_labels=True, **bufs):
    """pooled (N, C), w (K, C), b (K) f32 and labels (N) int64 (None: evaluation) -> dict of the requested `outputs`, one launch:
    logits (N, K), prob (N, K) softmax, pred (N) int64 arg-max (lowest index among ties), loss_rows (N) = logsumexp - logit[label],
    loss () = loss_weight * mean(loss_rows), dlogits (N, K) = loss_weight * (prob - onehot) / N.  Default outputs: logits, loss_rows, loss, dlogits with
    labels; logits, prob, pred without.  A buffer handed in by name (logits=..., prob=...) is written in place.  check_labels=False skips the range check
    (a host synchronisation) for labels that were checked before."""
    N, Cc = pooled.shape
    K = w.shape[0]
    assert w.shape == (K, Cc) and b.shape == (K,)
    if outputs is None:
        outputs = ("logits", "loss_rows", "loss", "dlogits") if labels is not None else ("logits", "prob", "pred")
    outputs = set(outputs) | set(bufs) | {"logits"}
    if not outputs <= set(_CLS_OUTPUTS):
        raise ValueError("cls_ce: unknown outputs %s" % sorted(outputs - set(_CLS_OUTPUTS)))
    if "loss" in outputs:
        outputs.add("loss_rows")
    if labels is None and outputs & {"loss_rows", "loss", "dlogits"}:
        raise ValueError("cls_ce: loss_rows / loss / dlogits need labels")
    if labels is not None and check_labels:
        _check_labels("cls_ce", labels, N, K)
    shapes = {"logits": ((N, K), torch.float32), "prob": ((N, K), torch.float32), "pred": ((N,), torch.int64), "loss_rows": ((N,), torch.float32),
              "loss": ((), torch.float32), "dlogits": ((N, K), torch.float32)}
    out = {}
    for name in _CLS_OUTPUTS:
        if name in outputs:
            t = bufs.get(name)
            shape, dtype = shapes[name]
            t = _scratch(shape, pooled.device, dtype) if t is None else t
            assert t.dtype == dtype and tuple(t.shape) == shape, name
            out[name] = t
    ptr = [_p(out.get(name)) for name in _CLS_OUTPUTS]
    counter = _cls_counter(pooled.device) if "loss" in out else None
    check(lib().mtp_cls_ce(_f32(pooled), _f32(w), _f32(b), _p(labels), float(loss_weight), *ptr, _p(counter), N, Cc, K, _s()), "mtp_cls_ce")
    return out


def cls_head_bwd(dlogits, pooled, w, dw, db, dpooled=None, accumulate=False):
    """dw (K, C) = / += dlogits^T . pooled, db (K) = / += column sums of dlogits, dpooled (N, C) = dlogits . w (None: not wanted); all f32, one launch"""
    N, K = dlogits.shape
    Cc = w.shape[1]
    assert pooled.shape == (N, Cc) and w.shape == dw.shape == (K, Cc) and db.shape == (K,) and (dpooled is None or dpooled.shape == (N, Cc))
    check(lib().mtp_cls_head_bwd(_f32(dlogits), _f32(pooled), _f32(w), _f32(dw), _f32(db), _f32(dpooled), N, Cc, K, int(accumulate), _s()),
          "mtp_cls_head_bwd")
    return dw, db, dpooled


def cls_hits(scores, labels, topk, counters, thr=0.0):
    """counters (len(topk) + 1) int64 += (hits for each k of topk, N).  scores (N, K) f32, labels (N) int64, topk ascending ints <= K.  The label's rank
    = #{j : s_j > s_label} + #{j < label : s_j == s_label}; a hit for k iff rank < k and s_label > thr (thr None: no threshold)."""
    N, K = scores.shape
    topk = [int(k) for k in topk]
    if not topk or len(topk) > CLS_MAX_TOPK or any(k < 1 for k in topk) or any(a >= b for a, b in zip(topk, topk[1:])):
        raise ValueError("cls_hits: topk must be 1 to %d ascending positive ints (got %s)" % (CLS_MAX_TOPK, topk))
    if topk[-1] > K:
        raise ValueError("cls_hits: topk %s exceeds the %d classes" % (tuple(topk), K))
    _check_labels("cls_hits", labels, N, K)
    assert counters.dtype == torch.int64 and counters.shape == (len(topk) + 1,)
    arr = (C.c_int32 * len(topk))(*topk)
    check(lib().mtp_cls_hits(_f32(scores), _p(labels), N, K, arr, len(topk), 0.0 if thr is None else float(thr), int(thr is not None), _p(counters), _s()),
          "mtp_cls_hits")
    return counters


# ------------------------------------------------------------------------------------------------ box operators (csrc/box_ops.hip)
NMS_MAX_BOXES = 32768      # 512 mask words per row: n x ceil(n / 64) x 8 bytes = 128 MB of workspace at the limit
_BOX_COLS = {_lib.BOX_ALIGNED: 4, _lib.BOX_ROTATED: 5}
ASSIGN_CALCULATOR = {"box": _lib.ASSIGN_BOX, "rbox2hbox": _lib.ASSIGN_RBOX2HBOX, "rotated": _lib.ASSIGN_ROTATED}
_ASSIGN_COLS = {_lib.ASSIGN_BOX: (4, 4), _lib.ASSIGN_RBOX2HBOX: (5, 4), _lib.ASSIGN_ROTATED: (5, 5)}


def _check_boxes(name, t, cols):
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != cols:
        raise TypeError("%s: boxes must be float32 of shape (n, %d), got %s %s" % (name, cols, t.dtype, tuple(t.shape)))


def box_iou(boxes1, boxes2, out=None, rotated=False, iof=False, aligned=False, eps=1e-6):
    """out (M, N) f32, or (M,) when aligned = IoU (IoF when iof) of boxes1 (M, 4 | 5) with boxes2 (N, 4 | 5): x1, y1, x2, y2, or cx, cy, w, h, theta when
    rotated.  M, N > 0."""
    kind = _lib.BOX_ROTATED if rotated else _lib.BOX_ALIGNED
    _check_boxes("box_iou", boxes1, _BOX_COLS[kind])
    _check_boxes("box_iou", boxes2, _BOX_COLS[kind])
    M, N = boxes1.shape[0], boxes2.shape[0]
    if aligned and M != N:
        raise ValueError("box_iou: aligned needs as many boxes1 as boxes2 (%d, %d)" % (M, N))
    shape = (M,) if aligned else (M, N)
    out = _scratch(shape, boxes1.device, torch.float32) if out is None else out
    assert out.dtype == torch.float32 and tuple(out.shape) == shape
    check(lib().mtp_box_iou(_f32(boxes1), _f32(boxes2), _f32(out), M, N, kind, int(iof), int(aligned), float(eps), _s()), "mtp_box_iou")
    return out


def check_nms_count(n):
    """the one refusal of too many boxes (ops_box asks before it sorts)"""
    if n > NMS_MAX_BOXES:
        raise ValueError("nms: %d boxes; at most %d (the suppression mask takes n x ceil(n / 64) x 8 bytes)" % (n, NMS_MAX_BOXES))


def nms_sorted(boxes, iou_threshold, groups=None, rotated=False, max_keep=None):
    """greedy NMS over boxes (n, 4 | 5) f32 ALREADY sorted by score, descending; groups (n) int64 or None: a pair suppresses only within one group.
    -> (keep (n) int64, count (1) int64) on the device: keep[:count] = the kept positions, ascending, at most max_keep.  Two launches, no sync."""
    kind = _lib.BOX_ROTATED if rotated else _lib.BOX_ALIGNED
    _check_boxes("nms_sorted", boxes, _BOX_COLS[kind])
    n = boxes.shape[0]
    check_nms_count(n)
    if groups is not None and (groups.dtype != torch.int64 or groups.shape != (n,)):
        raise TypeError("nms_sorted: groups must be int64 of shape (%d,)" % n)
    words = n * ((n + 63) // 64)
    mask = _scratch((words,), boxes.device, torch.int64)
    keep, count = _scratch((n,), boxes.device, torch.int64), _scratch((1,), boxes.device, torch.int64)
    check(lib().mtp_nms_mask(_f32(boxes), _p(groups), n, kind, float(iou_threshold), _p(mask), words * 8, _s()), "mtp_nms_mask")
    check(lib().mtp_nms_scan(_p(mask), n, n if max_keep is None or max_keep <= 0 else int(max_keep), _p(keep), _p(count), _s()), "mtp_nms_scan")
    return keep, count


def max_iou_assign(gts, priors, gt_labels, calculator, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True, gt_max_assign_all=True,
                   gt_inds=None, max_overlaps=None, labels=None):
    """MaxIoUAssigner.assign_wrt_overlaps without the K x N matrix: gts (K, 4 | 5), priors (N, 4 | 5) f32, gt_labels (K) int64, calculator 'box',
    'rbox2hbox' (rotated gts -> circumscribed boxes) or 'rotated'; neg_iou_thr a number or a (lo, hi) pair.  K, N > 0.
    -> gt_inds (N) int64, max_overlaps (N) f32, labels (N) int64"""
    calc = ASSIGN_CALCULATOR[calculator] if isinstance(calculator, str) else int(calculator)
    gc, pc = _ASSIGN_COLS[calc]
    _check_boxes("max_iou_assign", gts, gc)
    _check_boxes("max_iou_assign", priors, pc)
    K, N = gts.shape[0], priors.shape[0]
    if gt_labels.dtype != torch.int64 or gt_labels.shape != (K,):
        raise TypeError("max_iou_assign: gt_labels must be int64 of shape (%d,)" % K)
    lo, hi = (float(neg_iou_thr[0]), float(neg_iou_thr[1])) if isinstance(neg_iou_thr, (tuple, list)) else (0.0, float(neg_iou_thr))
    dev = priors.device
    gt_inds = _scratch((N,), dev, torch.int64) if gt_inds is None else gt_inds
    max_overlaps = _scratch((N,), dev, torch.float32) if max_overlaps is None else max_overlaps
    labels = _scratch((N,), dev, torch.int64) if labels is None else labels
    assert gt_inds.dtype == labels.dtype == torch.int64 and gt_inds.shape == labels.shape == max_overlaps.shape == (N,)
    ws = _scratch((K,), dev, torch.int64)
    check(lib().mtp_max_iou_assign(_f32(gts), _f32(priors), _p(gt_labels), K, N, calc, float(pos_iou_thr), lo, hi, float(min_pos_iou),
                                   int(bool(match_low_quality)), int(bool(gt_max_assign_all)), _p(gt_inds), _f32(max_overlaps), _p(labels), _p(ws), K * 8,
                                   _s()), "mtp_max_iou_assign")
    return gt_inds, max_overlaps, labels


# ------------------------------------------------------------------------------------------------ DOTA mAP metric (csrc/det_eval.hip)
DET_MAX_THRS, DET_MAX_CLASSES = _lib.DET_MAX_THRS, _lib.DET_MAX_CLASSES
DET_MAX_DETS = (1 << 32) - 2      # the ownership key keeps 2^32 - 1 - index in 32 bits and is never 0
DET_AP_MODE = {"11points": _lib.DET_AP_11POINTS, "area": _lib.DET_AP_AREA}
# np.arange(0, 1 + 1e-3, 0.1) as mmdet's average_precision evaluates it: 0.30000000000000004, 0.6000000000000001, 0.7000000000000001, ... -- a
# recall of exactly 3 / 10 does not reach the fourth point
DET_AP_POINTS = tuple(float(i) * 0.1 for i in range(_lib.DET_AP_POINTS))


def _det_thrs(name, iou_thrs):
    thrs = [float(t) for t in iou_thrs]
    if not 1 <= len(thrs) <= DET_MAX_THRS:
        raise ValueError("%s: 1 to %d IoU thresholds, got %d" % (name, DET_MAX_THRS, len(thrs)))
    return (C.c_float * len(thrs))(*thrs), len(thrs)


def _det_typed(name, what, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise TypeError("%s: %s must be %s of shape %s, got %s %s" % (name, what, str(dtype).replace("torch.", ""), tuple(shape), t.dtype, tuple(t.shape)))


def _det_count(name, D):
    if not 0 < D <= DET_MAX_DETS:
        raise ValueError("%s: 1 to 2^32 - 2 detections, got %d" % (name, D))


def _det_gts(name, gt_labels, gt_ignore, G):
    _det_typed(name, "gt_labels", gt_labels, torch.int64, (G,))
    _det_typed(name, "gt_ignore", gt_ignore, torch.uint8, (G,))


def det_match(det_boxes, det_scores, det_labels, det_img, gt_boxes, gt_labels, gt_ignore, gt_start, iou_thrs, best_iou=None, best_gt=None, winner=None):
    """detections (D, 5) f32 / scores (D) f32 / labels (D) / img (D) int64 against the gt table (G, 5) f32 / labels (G) int64 / ignore (G) uint8 stored
    image by image (non-ignored first), gt_start (I + 1) int64.  -> best_iou (D) f32, best_gt (D) int64 (-1: no gt of the label in the image),
    winner (T, G) int64 ownership keys (zeroed here).  One launch, no sync."""
    name = "det_match"
    _check_boxes(name, det_boxes, 5)
    _check_boxes(name, gt_boxes, 5)
    D, G, I = det_boxes.shape[0], gt_boxes.shape[0], gt_start.shape[0] - 1
    _det_count(name, D)
    thrs, T = _det_thrs(name, iou_thrs)
    _det_typed(name, "det_scores", det_scores, torch.float32, (D,))
    _det_typed(name, "det_labels", det_labels, torch.int64, (D,))
    _det_typed(name, "det_img", det_img, torch.int64, (D,))
    _det_gts(name, gt_labels, gt_ignore, G)
    if gt_start.dtype != torch.int64 or gt_start.dim() != 1 or I < 0:
        raise TypeError("det_match: gt_start must be int64 of shape (images + 1,)")
    dev = det_boxes.device
    best_iou = _scratch((D,), dev, torch.float32) if best_iou is None else best_iou
    best_gt = _scratch((D,), dev, torch.int64) if best_gt is None else best_gt
    winner = _scratch((T, G), dev, torch.int64).zero_() if winner is None else winner
    _det_typed(name, "best_iou", best_iou, torch.float32, (D,))
    _det_typed(name, "best_gt", best_gt, torch.int64, (D,))
    _det_typed(name, "winner", winner, torch.int64, (T, G))
    g = (lambda t: _p(t)) if G else (lambda t: None)
    check(lib().mtp_det_match(_f32(det_boxes), _f32(det_scores), _p(det_labels), _p(det_img), D, g(gt_boxes), g(gt_labels), g(gt_ignore), _p(gt_start), I,
                              G, thrs, T, _f32(best_iou), _p(best_gt), g(winner), T * G * 8, _s()), "mtp_det_match")
    return best_iou, best_gt, winner


def det_tpfp(det_scores, best_iou, best_gt, gt_labels, gt_ignore, iou_thrs, winner, num_classes, flags=None, num_gts=None):
    """-> flags (T, D) uint8 (1 true positive, 2 false positive, 0 matched to an ignored gt), num_gts (K) int64 = the non-ignored gts per label (zeroed
    here).  One launch, no sync."""
    name = "det_tpfp"
    D, G, K = det_scores.shape[0], gt_labels.shape[0], int(num_classes)
    _det_count(name, D)
    thrs, T = _det_thrs(name, iou_thrs)
    if not 0 < K <= DET_MAX_CLASSES:
        raise ValueError("%s: 1 to %d classes, got %d" % (name, DET_MAX_CLASSES, K))
    _det_typed(name, "det_scores", det_scores, torch.float32, (D,))
    _det_typed(name, "best_iou", best_iou, torch.float32, (D,))
    _det_typed(name, "best_gt", best_gt, torch.int64, (D,))
    _det_gts(name, gt_labels, gt_ignore, G)
    _det_typed(name, "winner", winner, torch.int64, (T, G))
    dev = det_scores.device
    flags = _scratch((T, D), dev, torch.uint8) if flags is None else flags
    num_gts = _scratch((K,), dev, torch.int64).zero_() if num_gts is None else num_gts
    _det_typed(name, "flags", flags, torch.uint8, (T, D))
    _det_typed(name, "num_gts", num_gts, torch.int64, (K,))
    g = (lambda t: _p(t)) if G else (lambda t: None)
    check(lib().mtp_det_tpfp(_f32(det_scores), _f32(best_iou), _p(best_gt), D, g(gt_labels), g(gt_ignore), G, thrs, T, g(winner), K, _p(flags), _p(num_gts),
                             _s()), "mtp_det_tpfp")
    return flags, num_gts


def det_ap(flags, order, cls_start, num_gts, mode="11points", curves=False, out=None):
    """flags (T, D) uint8 in table order; order (D) int64: the detections class by class, by descending score inside a class; cls_start (K + 1) int64;
    num_gts (K) int64.  -> ap (T, K) f32, num_dets (K) int64, last_recall (T, K) f64, and with curves the recall (T, D) f64 / precision (T, D) f32 by
    list position (else None, None).  One launch, no sync.  D may be 0."""
    name = "det_ap"
    if mode not in DET_AP_MODE:
        raise ValueError("det_ap: mode must be '11points' or 'area', got %r" % (mode,))
    if flags.dtype != torch.uint8 or flags.dim() != 2:
        raise TypeError("det_ap: flags must be uint8 of shape (T, D), got %s %s" % (flags.dtype, tuple(flags.shape)))
    T, D = flags.shape
    if not 1 <= T <= DET_MAX_THRS:
        raise ValueError("det_ap: 1 to %d IoU thresholds, got %d" % (DET_MAX_THRS, T))
    K = num_gts.shape[0]
    if not 0 < K <= DET_MAX_CLASSES or D > DET_MAX_DETS:
        raise ValueError("det_ap: 1 to %d classes and at most 2^32 - 2 detections, got %d and %d" % (DET_MAX_CLASSES, K, D))
    _det_typed(name, "order", order, torch.int64, (D,))
    _det_typed(name, "cls_start", cls_start, torch.int64, (K + 1,))
    _det_typed(name, "num_gts", num_gts, torch.int64, (K,))
    dev = num_gts.device
    if out is None:
        out = (_scratch((T, K), dev, torch.float32), _scratch((K,), dev, torch.int64), _scratch((T, K), dev, torch.float64),
               _scratch((T, D), dev, torch.float64) if curves else None, _scratch((T, D), dev, torch.float32) if curves else None)
    ap, num_dets, last_recall, recall, precision = out
    _det_typed(name, "ap", ap, torch.float32, (T, K))
    _det_typed(name, "num_dets", num_dets, torch.int64, (K,))
    _det_typed(name, "last_recall", last_recall, torch.float64, (T, K))
    if recall is not None:
        _det_typed(name, "recall", recall, torch.float64, (T, D))
    if precision is not None:
        _det_typed(name, "precision", precision, torch.float32, (T, D))
    d = (lambda t: _p(t)) if D else (lambda t: None)
    pts = (C.c_double * len(DET_AP_POINTS))(*DET_AP_POINTS)
    check(lib().mtp_det_ap(d(flags), d(order), _p(cls_start), _p(num_gts), D, K, T, DET_AP_MODE[mode], pts, _f32(ap), _p(num_dets), _p(last_recall),
                           None if recall is None else d(recall), None if precision is None else d(precision), _s()), "mtp_det_ap")
    return ap, num_dets, last_recall, recall, precision


# ------------------------------------------------------------------------------------------------ COCO-style metric (csrc/coco_eval.hip)
COCO_MAX_THRS, COCO_AREAS, COCO_MAX_DET_LEVELS, COCO_MAX_CLASSES = _lib.COCO_MAX_THRS, _lib.COCO_AREAS, _lib.COCO_MAX_DET_LEVELS, _lib.COCO_MAX_CLASSES
COCO_REC_THRS, COCO_MAX_CELL_GTS = _lib.COCO_REC_THRS, _lib.COCO_MAX_CELL_GTS
COCO_KIND = {"bbox": _lib.COCO_BBOX, "segm": _lib.COCO_SEGM}
COCO_MAX_DETS = (1 << 31) - 1
# COCOeval.Params.areaRng (all, small, medium, large; both ends inclusive) and recThrs
COCO_AREA_RNG = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))
COCO_REC_POINTS = tuple([i * (1.0 / 100) for i in range(100)] + [1.0])      # np.linspace(0, 1, 101) bit for bit: i * step, the last one the stop


def _i64s(values):
    return (C.c_int64 * len(values))(*[int(v) for v in values])


def _f64s(values):
    return (C.c_double * len(values))(*[float(v) for v in values])


def mask_pack(masks, words=None, areas=None):
    """masks (N, H, W) or (N, H * W), bool or uint8 -> words (N, ceil(H * W / 64)) int64 (bit p of word w = pixel 64 w + p, the tail zero) and areas (N)
    int64 (zeroed here).  One launch, no sync.  N may be 0."""
    name = "mask_pack"
    if masks.dtype not in (torch.bool, torch.uint8) or masks.dim() not in (2, 3):
        raise TypeError("mask_pack: masks must be bool or uint8 of shape (N, H, W) or (N, H * W), got %s %s" % (masks.dtype, tuple(masks.shape)))
    N, HW = masks.shape[0], int(masks.shape[1:].numel())
    if HW < 1:
        raise ValueError("mask_pack: empty masks (H * W = 0)")
    W, dev = (HW + 63) // 64, masks.device
    words = _scratch((N, W), dev, torch.int64) if words is None else words
    areas = _scratch((N,), dev, torch.int64).zero_() if areas is None else areas
    _det_typed(name, "words", words, torch.int64, (N, W))
    _det_typed(name, "areas", areas, torch.int64, (N,))
    if N:
        check(lib().mtp_mask_pack(_p(masks.view(torch.uint8) if masks.dtype == torch.bool else masks), N, HW, _p(words), _p(areas), _s()), "mtp_mask_pack")
    return words, areas


def coco_iou(kind, det, det_labels, gt, gt_labels, gt_crowd, det_start, gt_start, agnostic=False, iou=None, inter=None):
    """kind 'bbox': det / gt = boxes (D, 4) / (G, 4) f32 x1, y1, x2, y2.  kind 'segm': det / gt = (words, areas) of mask_pack, the same word count.
    labels int64, gt_crowd uint8.  det_start / gt_start: HOST sequences of n_img + 1 offsets, starting at 0, into the tables.  -> iou (sum D_i G_i) f64:
    image i's row-major (D_i, G_i) block at out_start[i]; inter (same layout) int64 for 'segm' else None; out_start (list).  No sync."""
    name = "coco_iou"
    if kind not in COCO_KIND:
        raise ValueError("coco_iou: kind must be 'bbox' or 'segm', got %r" % (kind,))
    D, G = det_labels.shape[0], gt_labels.shape[0]
    det_start, gt_start = [int(v) for v in det_start], [int(v) for v in gt_start]
    n_img = len(det_start) - 1
    if n_img < 0 or len(gt_start) != n_img + 1 or det_start[0] != 0 or gt_start[0] != 0 or det_start[-1] != D or gt_start[-1] != G:
        raise ValueError("coco_iou: det_start / gt_start must hold images + 1 offsets from 0 to the table sizes (%d, %d)" % (D, G))
    if any(b < a for a, b in zip(det_start, det_start[1:])) or any(b < a for a, b in zip(gt_start, gt_start[1:])):
        raise ValueError("coco_iou: offsets must not decrease")
    _det_typed(name, "det_labels", det_labels, torch.int64, (D,))
    _det_gts(name, gt_labels, gt_crowd, G)
    W, boxes, words = 0, (None, None), (None, None, None, None)
    if kind == "bbox":
        _check_boxes(name, det, 4)
        _check_boxes(name, gt, 4)
        if det.shape[0] != D or gt.shape[0] != G:
            raise TypeError("coco_iou: %d / %d boxes for %d / %d labels" % (det.shape[0], gt.shape[0], D, G))
        boxes = (det, gt)
    else:
        (dw, da), (gw, ga) = det, gt
        W = dw.shape[1] if dw.dim() == 2 else -1
        _det_typed(name, "det words", dw, torch.int64, (D, W))
        _det_typed(name, "gt words", gw, torch.int64, (G, W))
        _det_typed(name, "det areas", da, torch.int64, (D,))
        _det_typed(name, "gt areas", ga, torch.int64, (G,))
        if W < 1:
            raise ValueError("coco_iou: masks without words")
        words = (dw, da, gw, ga)
    out_start = [0]
    for i in range(n_img):
        out_start.append(out_start[-1] + (det_start[i + 1] - det_start[i]) * (gt_start[i + 1] - gt_start[i]))
    n, dev = out_start[-1], det_labels.device
    iou = _scratch((n,), dev, torch.float64) if iou is None else iou
    _det_typed(name, "iou", iou, torch.float64, (n,))
    if kind == "segm":
        inter = _scratch((n,), dev, torch.int64) if inter is None else inter
        _det_typed(name, "inter", inter, torch.int64, (n,))
    else:
        inter = None
    q = lambda t: _p(t) if (t is not None and t.numel()) else None      # noqa: E731
    if n:
        check(lib().mtp_coco_iou(COCO_KIND[kind], q(boxes[0]), q(words[0]), q(words[1]), q(det_labels), D, q(boxes[1]), q(words[2]), q(words[3]),
                                 q(gt_labels), q(gt_crowd), G, W, int(bool(agnostic)), n_img, _i64s(det_start), _i64s(gt_start), _i64s(out_start), _p(iou),
                                 q(inter), n, _s()), "mtp_coco_iou")
    return iou, inter, out_start


def _coco_thrs(name, iou_thrs):
    thrs = [float(t) for t in iou_thrs]
    if not 1 <= len(thrs) <= COCO_MAX_THRS:
        raise ValueError("%s: 1 to %d IoU thresholds, got %d" % (name, COCO_MAX_THRS, len(thrs)))
    return thrs


def _coco_max_dets(name, max_dets):
    mds = [int(m) for m in max_dets]
    if not 1 <= len(mds) <= COCO_MAX_DET_LEVELS or any(m < 1 or m > COCO_MAX_DETS for m in mds):
        raise ValueError("%s: 1 to %d positive maxDets, got %r" % (name, COCO_MAX_DET_LEVELS, mds))
    return mds


def coco_match(iou, det_row, det_area, det_cell_start, gt_order, gt_col, gt_crowd, gt_ig, gt_cell_start, num_classes, iou_thrs, max_det,
               area_rng=COCO_AREA_RNG, max_cell_gts=0, out=None):
    """COCOeval.evaluateImg on the tables of include/mtp_hip.h (mtp_coco_match): the (D) detection tables in list order (cell by cell, by descending
    score), det_cell_start / gt_cell_start (cells + 1) with cells = images x num_classes, gt_order / gt_ig (4, G).  max_cell_gts: the caller's
    host-known bound on the gts of one cell (the largest image's gt count), refused beyond COCO_MAX_CELL_GTS.  -> matched, ignored (4, T, D) uint8,
    rank (D) int32, npig (K, 4) int64 (zeroed here).  One launch, no sync."""
    name = "coco_match"
    thrs, A = _coco_thrs(name, iou_thrs), COCO_AREAS
    T, K, D, G, cells = len(thrs), int(num_classes), det_row.shape[0], gt_col.shape[0], det_cell_start.shape[0] - 1
    if not 0 < K <= COCO_MAX_CLASSES or cells < 0 or cells % K:
        raise ValueError("%s: 1 to %d classes and images x classes cells, got %d classes, %d cells" % (name, COCO_MAX_CLASSES, K, cells))
    if int(max_cell_gts) > COCO_MAX_CELL_GTS:
        raise ValueError("%s: %d gts in one image; at most %d per (image, category)" % (name, max_cell_gts, COCO_MAX_CELL_GTS))
    if D > COCO_MAX_DETS or G > COCO_MAX_DETS or not 1 <= int(max_det) <= COCO_MAX_DETS:
        raise ValueError("%s: at most 2^31 - 1 detections, gts and max_det" % name)
    if len(area_rng) != A:
        raise ValueError("%s: %d area ranges" % (name, A))
    if iou.dtype != torch.float64 or iou.dim() != 1:
        raise TypeError("%s: iou must be float64 of shape (n,)" % name)
    _det_typed(name, "det_row", det_row, torch.int64, (D,))
    _det_typed(name, "det_area", det_area, torch.float64, (D,))
    _det_typed(name, "det_cell_start", det_cell_start, torch.int64, (cells + 1,))
    _det_typed(name, "gt_cell_start", gt_cell_start, torch.int64, (cells + 1,))
    _det_typed(name, "gt_order", gt_order, torch.int64, (A, G))
    _det_typed(name, "gt_ig", gt_ig, torch.uint8, (A, G))
    _det_typed(name, "gt_col", gt_col, torch.int64, (G,))
    _det_typed(name, "gt_crowd", gt_crowd, torch.uint8, (G,))
    dev = det_cell_start.device
    if out is None:
        out = (_scratch((A, T, D), dev, torch.uint8), _scratch((A, T, D), dev, torch.uint8), _scratch((D,), dev, torch.int32),
               _scratch((K, A), dev, torch.int64).zero_())
    matched, ignored, rank, npig = out
    _det_typed(name, "matched", matched, torch.uint8, (A, T, D))
    _det_typed(name, "ignored", ignored, torch.uint8, (A, T, D))
    _det_typed(name, "rank", rank, torch.int32, (D,))
    _det_typed(name, "npig", npig, torch.int64, (K, A))
    q = lambda t: _p(t) if t.numel() else None      # noqa: E731
    rng = _f64s([v for lo_hi in area_rng for v in lo_hi])
    if cells:
        check(lib().mtp_coco_match(q(iou), iou.numel(), q(det_row), q(det_area), _p(det_cell_start), D, q(gt_order), q(gt_col), q(gt_crowd), q(gt_ig),
                                   _p(gt_cell_start), G, cells, K, _f64s(thrs), T, rng, int(max_det), q(matched), q(ignored), q(rank), _p(npig), _s()),
              "mtp_coco_match")
    return matched, ignored, rank, npig


def coco_accumulate(matched, ignored, rank, score, order, cls_start, npig, max_dets, rec_thrs=COCO_REC_POINTS, out=None):
    """COCOeval.accumulate: matched / ignored (4, T, D) uint8, rank (D) int32 and score (D) f32 by list position; order (D) int64: list positions
    category by category, by descending score; cls_start (K + 1); npig (K, 4) int64.  -> precision (T, 101, K, 4, M) f64, scores (same shape) f64,
    recall (T, K, 4, M) f64.  One launch, no sync.  D may be 0."""
    name = "coco_accumulate"
    mds, A, R = _coco_max_dets(name, max_dets), COCO_AREAS, COCO_REC_THRS
    if matched.dtype != torch.uint8 or matched.dim() != 3 or matched.shape[0] != A:
        raise TypeError("%s: matched must be uint8 of shape (4, T, D), got %s %s" % (name, matched.dtype, tuple(matched.shape)))
    T, D, K, M = matched.shape[1], matched.shape[2], npig.shape[0], len(mds)
    if not 1 <= T <= COCO_MAX_THRS or not 0 < K <= COCO_MAX_CLASSES or D > COCO_MAX_DETS:
        raise ValueError("%s: 1 to %d thresholds, 1 to %d classes, at most 2^31 - 1 detections; got %d, %d, %d" % (name, COCO_MAX_THRS, COCO_MAX_CLASSES, T, K, D))
    if len(rec_thrs) != R:
        raise ValueError("%s: %d recall thresholds" % (name, R))
    _det_typed(name, "ignored", ignored, torch.uint8, (A, T, D))
    _det_typed(name, "rank", rank, torch.int32, (D,))
    _det_typed(name, "score", score, torch.float32, (D,))
    _det_typed(name, "order", order, torch.int64, (D,))
    _det_typed(name, "cls_start", cls_start, torch.int64, (K + 1,))
    _det_typed(name, "npig", npig, torch.int64, (K, A))
    dev = npig.device
    if out is None:
        out = (_scratch((T, R, K, A, M), dev, torch.float64), _scratch((T, R, K, A, M), dev, torch.float64), _scratch((T, K, A, M), dev, torch.float64))
    precision, scores, recall = out
    _det_typed(name, "precision", precision, torch.float64, (T, R, K, A, M))
    _det_typed(name, "scores", scores, torch.float64, (T, R, K, A, M))
    _det_typed(name, "recall", recall, torch.float64, (T, K, A, M))
    q = lambda t: _p(t) if t.numel() else None      # noqa: E731
    check(lib().mtp_coco_accumulate(q(matched), q(ignored), q(rank), q(score), q(order), _p(cls_start), _p(npig), D, K, T, (C.c_int32 * M)(*mds), M,
                                    _f64s(rec_thrs), _p(precision), _p(scores), _p(recall), _s()), "mtp_coco_accumulate")
    return precision, scores, recall


# ------------------------------------------------------------------------------------------------ oriented RPN (csrc/rpn.hip)
RPN_MAX_LEVELS = _lib.RPN_MAX_LEVELS
RPN_DELTAS = 6


def rpn_map_nchw(t):
    """a level's map in mmdet's layout (N, A * C, H, W), contiguous f32 -> (tensor, element offset, strides (image, channel, y, x))"""
    N, Cc, H, W = t.shape
    return t, 0, (Cc * H * W, H * W, W, 1)


def rpn_map_rows(t, H, W, col0=0, row0=0):
    """a level's map in the engines' row layout: rows row0 .. row0 + N * H * W of t (., ld), channel c at column col0 + c"""
    ld = t.shape[1]
    return t, row0 * ld + col0, (H * W * ld, 1, W * ld, ld)


def _rpn_codec(means, stds):
    m, s = [float(v) for v in means], [float(v) for v in stds]
    if len(m) != RPN_DELTAS or len(s) != RPN_DELTAS or min(s) <= 0:
        raise ValueError("the midpoint-offset coder takes 6 means and 6 positive stds")
    return (C.c_float * 6)(*m), (C.c_float * 6)(*s)


def _rpn_levels(cls_maps, reg_maps, sizes, A, images, dcls=None, dreg=None, keep_counts=None, deltas=RPN_DELTAS):
    """-> (mtp_rpn_level array, number of anchors); every address a kernel can form from the strides lies inside its tensor.  deltas: the reg
    channels per anchor (6 for the oriented head, 4 for the horizontal one)"""
    n = len(sizes)
    if not 1 <= n <= RPN_MAX_LEVELS or len(cls_maps) != n or len(reg_maps) != n:
        raise ValueError("rpn: 1 .. %d levels, one cls and one reg map each" % RPN_MAX_LEVELS)
    arr = (_lib.RpnLevel * n)()
    total = 0

    def addr(m, channels, H, W, like=None):
        t, off, st = m
        if t.dtype != torch.float32:
            raise TypeError("rpn: the maps are float32")
        if like is not None and (like[1] != off or tuple(like[2]) != tuple(st) or like[0].numel() != t.numel()):
            raise ValueError("rpn: a gradient map has the layout of its map")
        last = off + (images - 1) * st[0] + (channels - 1) * st[1] + (H - 1) * st[2] + (W - 1) * st[3]
        if off < 0 or min(st) < 0 or last >= t.numel():
            raise ValueError("rpn: a map's strides reach past its tensor")
        return _p(t) + 4 * off

    for i, (H, W) in enumerate(sizes):
        lv = arr[i]
        lv.cls, lv.reg = addr(cls_maps[i], A, H, W), addr(reg_maps[i], A * deltas, H, W)
        if dcls is not None:
            lv.dcls, lv.dreg = addr(dcls[i], A, H, W, cls_maps[i]), addr(dreg[i], A * deltas, H, W, reg_maps[i])
        lv.H, lv.W = H, W
        lv.keep_count = 0 if keep_counts is None else int(keep_counts[i])
        lv.cls_stride, lv.reg_stride = (C.c_int64 * 4)(*cls_maps[i][2]), (C.c_int64 * 4)(*reg_maps[i][2])
        total += H * W * A
    return arr, total


def rpn_anchors(base_anchors, H, W, stride, pad_shape, img_shape, allowed_border=0, priors=None, flags=None):
    """base_anchors (A, 4) f32 on the device -> priors (H W A, 4) f32, inside flags (H W A) uint8.  stride: (w, h)."""
    _check_boxes("rpn_anchors", base_anchors, 4)
    A = base_anchors.shape[0]
    n = H * W * A
    priors = _scratch((n, 4), base_anchors.device, torch.float32) if priors is None else priors
    flags = _scratch((n,), base_anchors.device, torch.uint8) if flags is None else flags
    assert tuple(priors.shape) == (n, 4) and flags.dtype == torch.uint8 and tuple(flags.shape) == (n,)
    check(lib().mtp_rpn_anchors(_f32(base_anchors), A, H, W, int(stride[0]), int(stride[1]), int(pad_shape[0]), int(pad_shape[1]), int(img_shape[0]),
                                int(img_shape[1]), float(allowed_border), _f32(priors), _p(flags), _s()), "mtp_rpn_anchors")
    return priors, flags


def rpn_loss(cls_maps, reg_maps, sizes, A, priors, gts, samples, sample_gt, n_pos, n_neg, means, stds, beta, cls_weight=1.0, bbox_weight=1.0,
             dcls=None, dreg=None, loss_cls=None, loss_bbox=None):
    """Targets and loss of the oriented RPN for the whole batch (mtp_rpn_loss): two launches, no host synchronisation.  cls_maps / reg_maps: per level
    an rpn_map_nchw / rpn_map_rows triple; sizes: per level (H, W); priors (sum H W A, 4); gts (K, 5) of all images (K may be 0); samples, sample_gt
    (images, S) int64; n_pos, n_neg (images) int64.  dcls / dreg: gradient maps in the maps' layout, ZEROED by the caller (both or neither).
    -> (loss_cls (levels), loss_bbox (levels)) f32"""
    _check_boxes("rpn_loss", priors, 4)
    _check_boxes("rpn_loss", gts, 5)
    images, S = samples.shape
    if (dcls is None) != (dreg is None):
        raise ValueError("rpn_loss: dcls and dreg come together")
    arr, total = _rpn_levels(cls_maps, reg_maps, sizes, A, images, dcls, dreg)
    if priors.shape[0] != total:
        raise ValueError("rpn_loss: %d priors for %d anchors" % (priors.shape[0], total))
    for t, shape in ((samples, (images, S)), (sample_gt, (images, S)), (n_pos, (images,)), (n_neg, (images,))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape:
            raise TypeError("rpn_loss: samples, sample_gt (images, S) and n_pos, n_neg (images) are int64")
    dev, n = priors.device, len(sizes)
    loss_cls = _scratch((n,), dev, torch.float32) if loss_cls is None else loss_cls
    loss_bbox = _scratch((n,), dev, torch.float32) if loss_bbox is None else loss_bbox
    assert tuple(loss_cls.shape) == tuple(loss_bbox.shape) == (n,)
    wb = lib().mtp_rpn_loss_workspace_bytes(images, S)
    ws = _scratch((wb // 4,), dev, torch.float32)
    m, s = _rpn_codec(means, stds)
    K = gts.shape[0]
    check(lib().mtp_rpn_loss(arr, n, A, _f32(priors), total, _f32(gts) if K else None, K, _p(samples), _p(sample_gt), _p(n_pos), _p(n_neg), images, S, m, s,
                             float(beta), float(cls_weight), float(bbox_weight), _f32(loss_cls), _f32(loss_bbox), _p(ws), wb, _s()), "mtp_rpn_loss")
    return loss_cls, loss_bbox


def rpn_proposals(cls_maps, reg_maps, sizes, A, priors, keep, keep_counts, means, stds, min_bbox_size=0.0, out=None):
    """keep (images, T) int64, T = sum(keep_counts): per level the kept anchors (indices into the level's own H W A), level after level.
    -> scores (images, T) f32, rboxes (images, T, 5), hboxes (images, T, 4), level_ids (images, T) int64, valid (images, T) uint8.  One launch."""
    _check_boxes("rpn_proposals", priors, 4)
    images, T = keep.shape
    if keep.dtype != torch.int64 or T != sum(int(k) for k in keep_counts) or T == 0:
        raise TypeError("rpn_proposals: keep must be int64 of shape (images, sum(keep_counts) > 0)")
    arr, total = _rpn_levels(cls_maps, reg_maps, sizes, A, images, keep_counts=keep_counts)
    if priors.shape[0] != total:
        raise ValueError("rpn_proposals: %d priors for %d anchors" % (priors.shape[0], total))
    dev = priors.device
    if out is None:
        out = (_scratch((images, T), dev, torch.float32), _scratch((images, T, 5), dev, torch.float32), _scratch((images, T, 4), dev, torch.float32),
               _scratch((images, T), dev, torch.int64), _scratch((images, T), dev, torch.uint8))
    scores, rboxes, hboxes, level_ids, valid = out
    assert tuple(scores.shape) == tuple(level_ids.shape) == tuple(valid.shape) == (images, T) and level_ids.dtype == torch.int64 and valid.dtype == torch.uint8
    assert tuple(rboxes.shape) == (images, T, 5) and tuple(hboxes.shape) == (images, T, 4)
    m, s = _rpn_codec(means, stds)
    check(lib().mtp_rpn_proposals(arr, len(sizes), A, _f32(priors), total, _p(keep), images, m, s, float(min_bbox_size), _f32(scores), _f32(rboxes),
                                  _f32(hboxes), _p(level_ids), _p(valid), _s()), "mtp_rpn_proposals")
    return scores, rboxes, hboxes, level_ids, valid


def rpn_encode(priors, gts, means, stds, out=None):
    """midpoint-offset encode: priors (n, 4), gts (n, 5) -> deltas (n, 6)"""
    _check_boxes("rpn_encode", priors, 4)
    _check_boxes("rpn_encode", gts, 5)
    n = priors.shape[0]
    assert gts.shape[0] == n and n > 0
    out = _scratch((n, 6), priors.device, torch.float32) if out is None else out
    assert tuple(out.shape) == (n, 6)
    m, s = _rpn_codec(means, stds)
    check(lib().mtp_rpn_encode(_f32(priors), _f32(gts), m, s, n, _f32(out), _s()), "mtp_rpn_encode")
    return out


def rpn_decode(priors, deltas, means, stds, out=None):
    """midpoint-offset decode: priors (n, 4), deltas (n, 6) -> rotated boxes (n, 5), w >= h, theta in [-pi/2, pi/2)"""
    _check_boxes("rpn_decode", priors, 4)
    _check_boxes("rpn_decode", deltas, 6)
    n = priors.shape[0]
    assert deltas.shape[0] == n and n > 0
    out = _scratch((n, 5), priors.device, torch.float32) if out is None else out
    assert tuple(out.shape) == (n, 5)
    m, s = _rpn_codec(means, stds)
    check(lib().mtp_rpn_decode(_f32(priors), _f32(deltas), m, s, n, _f32(out), _s()), "mtp_rpn_decode")
    return out


# ------------------------------------------------------------------------------------------------ oriented RoI head (csrc/roi_head.hip)
ROI_MAX_LEVELS = _lib.ROI_MAX_LEVELS
ROI_DELTAS = 5
ROI_MAX_POINTS = 1024      # out_size^2 * sample_num^2: the sample points of one RoI live in LDS


def _roi_codec(means, stds):
    m, s = [float(v) for v in means], [float(v) for v in stds]
    if len(m) != ROI_DELTAS or len(s) != ROI_DELTAS or min(s) <= 0:
        raise ValueError("the delta-xywht coder takes 5 means and 5 positive stds")
    return (C.c_float * 5)(*m), (C.c_float * 5)(*s)


def _roi_levels(maps, sizes, scales, images, channels, grads=False):
    """maps: per level an rpn_map_nchw / rpn_map_rows triple (the gradient maps when grads) -> mtp_roi_level array; every address a kernel can form
    from the strides lies inside its tensor"""
    n = len(sizes)
    if not 1 <= n <= ROI_MAX_LEVELS or len(scales) != n or (maps is not None and len(maps) != n):
        raise ValueError("roi_align_rotated: 1 .. %d levels, one map and one spatial scale each" % ROI_MAX_LEVELS)
    arr = (_lib.RoiLevel * n)()
    for i, (H, W) in enumerate(sizes):
        lv = arr[i]
        lv.H, lv.W, lv.spatial_scale = int(H), int(W), float(scales[i])
        if maps is None:
            continue
        t, off, st = maps[i]
        if t.dtype != torch.float32:
            raise TypeError("roi_align_rotated: the maps are float32")
        last = off + (images - 1) * st[0] + (channels - 1) * st[1] + (H - 1) * st[2] + (W - 1) * st[3]
        if off < 0 or min(st) < 0 or last >= t.numel():
            raise ValueError("roi_align_rotated: a map's strides reach past its tensor")
        if grads:
            lv.dmap = _p(t) + 4 * off
        else:
            lv.map = _p(t) + 4 * off
        lv.stride = (C.c_int64 * 4)(*st)
    return arr


def _roi_check(name, rois, roi_levels, valid, out_size, sample_num):
    if rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] != 6 or rois.shape[0] == 0:
        raise TypeError("%s: rois must be float32 of shape (R > 0, 6): image, cx, cy, w, h, theta" % name)
    R = rois.shape[0]
    if out_size < 1 or sample_num < 1 or out_size * out_size * sample_num * sample_num > ROI_MAX_POINTS:
        raise ValueError("%s: out_size^2 * sample_num^2 must lie in 1 .. %d" % (name, ROI_MAX_POINTS))
    if roi_levels is not None and (roi_levels.dtype != torch.int32 or tuple(roi_levels.shape) != (R,)):
        raise TypeError("%s: roi_levels must be int32 of shape (R,)" % name)
    per = 0
    if valid is not None:
        if valid.dtype != torch.int64 or valid.dim() != 1 or valid.numel() == 0 or R % valid.numel():
            raise TypeError("%s: valid must be int64 (groups,) with R a multiple of groups" % name)
        per = R // valid.numel()
    return R, per


def roi_align_rotated_fwd(maps, sizes, scales, channels, images, rois, out_size=7, sample_num=2, clockwise=False, finest_scale=56.0, roi_levels=None,
                          valid=None, out=None, levels_out=None):
    """RoIAlignRotated (aligned) of all RoIs over all levels in one launch.  maps: per level an rpn_map_nchw / rpn_map_rows triple; sizes (H, W) and
    scales (1 / stride) per level; rois (R, 6) f32; roi_levels (R) int32 overrides the level map; valid (groups) int64: slot r is in use iff
    r % (R / groups) < valid[r // (R / groups)].  -> out (R, out_size^2, channels) f32, bin-major and channel-last"""
    R, per = _roi_check("roi_align_rotated_fwd", rois, roi_levels, valid, out_size, sample_num)
    arr = _roi_levels(maps, sizes, scales, images, channels)
    shape = (R, out_size * out_size, channels)
    out = _scratch(shape, rois.device, torch.float32) if out is None else out
    assert tuple(out.shape) == shape and (levels_out is None or (levels_out.dtype == torch.int32 and tuple(levels_out.shape) == (R,)))
    check(lib().mtp_roi_align_rotated_fwd(arr, len(sizes), images, channels, _f32(rois), _p(roi_levels), _p(valid), R, per, out_size, sample_num,
                                          int(bool(clockwise)), float(finest_scale), _f32(out), _p(levels_out), _s()), "mtp_roi_align_rotated_fwd")
    return out


def roi_align_rotated_bwd(dout, dmaps, sizes, scales, channels, images, rois, out_size=7, sample_num=2, clockwise=False, finest_scale=56.0,
                          roi_levels=None, valid=None, accumulate=False):
    """the gradient of roi_align_rotated_fwd with respect to the maps, deterministic: entries, a stable sort of their pixel keys, one owner per
    touched pixel.  dout (R, out_size^2, channels); dmaps: per level a triple in the maps' layout.  Only the touched pixels are written: stored, or
    added to what is there when accumulate -- the caller zeroes the maps otherwise.  No gradient to the RoIs (mmcv has none)."""
    R, per = _roi_check("roi_align_rotated_bwd", rois, roi_levels, valid, out_size, sample_num)
    if dout.dtype != torch.float32 or tuple(dout.shape) != (R, out_size * out_size, channels):
        raise TypeError("roi_align_rotated_bwd: dout must be float32 of shape (R, out_size^2, channels)")
    n = lib().mtp_roi_align_rotated_entries(R, out_size, sample_num)
    keys, weights = _scratch((n,), rois.device, torch.int64), _scratch((n,), rois.device, torch.float32)
    geo = _roi_levels(None, sizes, scales, images, channels)
    check(lib().mtp_roi_align_rotated_bwd_entries(geo, len(sizes), images, _f32(rois), _p(roi_levels), _p(valid), R, per, out_size, sample_num,
                                                  int(bool(clockwise)), float(finest_scale), _p(keys), _f32(weights), _s()),
          "mtp_roi_align_rotated_bwd_entries")
    skeys, order = torch.sort(keys, stable=True)
    arr = _roi_levels(dmaps, sizes, scales, images, channels, grads=True)
    check(lib().mtp_roi_align_rotated_bwd_gather(arr, len(sizes), images, channels, _f32(dout), _p(skeys.contiguous()), _p(order.contiguous()), _f32(weights),
                                                 R, out_size, sample_num, int(bool(accumulate)), _s()), "mtp_roi_align_rotated_bwd_gather")
    return dmaps


def rbox_delta_encode(priors, gts, means, stds, out=None):
    """DeltaXYWHTRBBoxCoder ('le90', edge_swap, proj_xy) encode: priors (n, 5), gts (n, 5) -> deltas (n, 5)"""
    _check_boxes("rbox_delta_encode", priors, 5)
    _check_boxes("rbox_delta_encode", gts, 5)
    n = priors.shape[0]
    assert gts.shape[0] == n and n > 0
    out = _scratch((n, 5), priors.device, torch.float32) if out is None else out
    assert tuple(out.shape) == (n, 5)
    m, s = _roi_codec(means, stds)
    check(lib().mtp_rbox_delta_encode(_f32(priors), _f32(gts), m, s, n, _f32(out), _s()), "mtp_rbox_delta_encode")
    return out


def rbox_delta_decode(priors, deltas, means, stds, out=None):
    """decode: priors (n, 5), deltas (n, 5) -> rotated boxes (n, 5), w >= h, theta in [-pi/2, pi/2)"""
    _check_boxes("rbox_delta_decode", priors, 5)
    _check_boxes("rbox_delta_decode", deltas, 5)
    n = priors.shape[0]
    assert deltas.shape[0] == n and n > 0
    out = _scratch((n, 5), priors.device, torch.float32) if out is None else out
    assert tuple(out.shape) == (n, 5)
    m, s = _roi_codec(means, stds)
    check(lib().mtp_rbox_delta_decode(_f32(priors), _f32(deltas), m, s, n, _f32(out), _s()), "mtp_rbox_delta_decode")
    return out


def _roi_rows(name, t, cols):
    """a (rows, >= cols) f32 view whose rows are ld apart -> (address, ld)"""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < cols or t.stride(1) != 1 or not t.is_cuda:
        raise TypeError("%s: expected float32 device rows of at least %d columns" % (name, cols))
    return t.data_ptr(), t.stride(0)


def roi_loss(cls_score, bbox_pred, num_classes, rois, gts, gt_labels, sample_gt, n_pos, n_neg, means, stds, beta=1.0, cls_weight=1.0, bbox_weight=1.0,
             dcls=None, dreg=None, losses=None):
    """Targets and losses of the RoI head for the whole batch (mtp_roi_loss): two launches, no host synchronisation.  cls_score (images * S,
    num_classes + 1) and bbox_pred (images * S, 5): rows of a wider buffer are fine (column slices); rois (images * S, 5); gts (G, 5), gt_labels (G)
    of all images; sample_gt (images, S), n_pos, n_neg (images) int64.  dcls / dreg: the gradients, in the layout of their inputs.
    -> losses (3) f32: loss_cls, loss_bbox, acc in percent"""
    images, S = sample_gt.shape
    R = images * S
    _check_boxes("roi_loss", rois, 5)
    _check_boxes("roi_loss", gts, 5)
    if rois.shape[0] != R or cls_score.shape[0] != R or bbox_pred.shape[0] != R:
        raise ValueError("roi_loss: %d rows for %d x %d slots" % (rois.shape[0], images, S))
    G = gts.shape[0]
    for t, shape in ((sample_gt, (images, S)), (n_pos, (images,)), (n_neg, (images,)), (gt_labels, (G,))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape:
            raise TypeError("roi_loss: sample_gt (images, S), n_pos, n_neg (images) and gt_labels (G) are int64")
    (pc, ldc), (pr, ldr) = _roi_rows("roi_loss", cls_score, num_classes + 1), _roi_rows("roi_loss", bbox_pred, 5)
    if (dcls is None) != (dreg is None):
        raise ValueError("roi_loss: dcls and dreg come together")
    pdc = pdr = None
    if dcls is not None:
        (pdc, a), (pdr, b) = _roi_rows("roi_loss", dcls, num_classes + 1), _roi_rows("roi_loss", dreg, 5)
        if a != ldc or b != ldr or dcls.shape[0] != R or dreg.shape[0] != R:
            raise ValueError("roi_loss: a gradient has the layout of its input")
    dev = rois.device
    losses = _scratch((3,), dev, torch.float32) if losses is None else losses
    assert tuple(losses.shape) == (3,)
    wb = lib().mtp_roi_loss_workspace_bytes(images, S)
    ws = _scratch((wb // 4,), dev, torch.float32)
    m, s = _roi_codec(means, stds)
    check(lib().mtp_roi_loss(pc, ldc, pr, ldr, int(num_classes), _f32(rois), _f32(gts) if G else None, _p(gt_labels) if G else None, G, _p(sample_gt),
                             _p(n_pos), _p(n_neg), images, S, m, s, float(beta), float(cls_weight), float(bbox_weight), _f32(losses), pdc, pdr, _p(ws), wb,
                             _s()), "mtp_roi_loss")
    return losses


def roi_predict(cls_score, bbox_pred, num_classes, rois, means, stds, score_thr=0.0, out=None):
    """per RoI the softmax scores (R, num_classes), the decoded box (R, 5) and the score > score_thr flags (R, num_classes) uint8: one launch"""
    _check_boxes("roi_predict", rois, 5)
    R = rois.shape[0]
    if R == 0 or cls_score.shape[0] != R or bbox_pred.shape[0] != R:
        raise ValueError("roi_predict: R > 0 rows of scores, deltas and rois")
    (pc, ldc), (pr, ldr) = _roi_rows("roi_predict", cls_score, num_classes + 1), _roi_rows("roi_predict", bbox_pred, 5)
    dev = rois.device
    if out is None:
        out = (_scratch((R, num_classes), dev, torch.float32), _scratch((R, 5), dev, torch.float32), _scratch((R, num_classes), dev, torch.uint8))
    scores, boxes, flags = out
    assert tuple(scores.shape) == tuple(flags.shape) == (R, num_classes) and tuple(boxes.shape) == (R, 5) and flags.dtype == torch.uint8
    m, s = _roi_codec(means, stds)
    check(lib().mtp_roi_predict(pc, ldc, pr, ldr, int(num_classes), _f32(rois), R, m, s, float(score_thr), _f32(scores), _f32(boxes), _p(flags), _s()),
          "mtp_roi_predict")
    return scores, boxes, flags


# ------------------------------------------------------------------------------------------------ the mask branch (csrc/mask_head.hip)
ROI_ALIGN_MAX_OUT = 32          # out_size of roi_align_fwd / _bwd
ROI_ALIGN_MAX_SAMPLING = 64     # a fixed sampling_ratio; 0 is the adaptive grid


def _roi_align_check(name, rois, roi_levels, valid, out_size, sampling_ratio):
    if rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] == 0:
        raise TypeError("%s: rois must be float32 of shape (R > 0, 5): image, x1, y1, x2, y2" % name)
    R = rois.shape[0]
    if not 1 <= out_size <= ROI_ALIGN_MAX_OUT or not 0 <= sampling_ratio <= ROI_ALIGN_MAX_SAMPLING:
        raise ValueError("%s: out_size in 1 .. %d, sampling_ratio in 0 .. %d" % (name, ROI_ALIGN_MAX_OUT, ROI_ALIGN_MAX_SAMPLING))
    if roi_levels is not None and (roi_levels.dtype != torch.int32 or tuple(roi_levels.shape) != (R,)):
        raise TypeError("%s: roi_levels must be int32 of shape (R,)" % name)
    per = 0
    if valid is not None:
        if valid.dtype != torch.int64 or valid.dim() != 1 or valid.numel() == 0 or R % valid.numel():
            raise TypeError("%s: valid must be int64 (groups,) with R a multiple of groups" % name)
        per = R // valid.numel()
    return R, per


def roi_align_fwd(maps, sizes, scales, channels, images, rois, out_size=14, sampling_ratio=0, aligned=True, finest_scale=56.0, roi_levels=None,
                  valid=None, out=None, levels_out=None):
    """RoIAlign (mmcv roi_align, 'avg') of all RoIs over all levels in one launch.  maps: per level an rpn_map_nchw / rpn_map_rows triple; sizes
    (H, W) and scales (1 / stride) per level; rois (R, 5) f32: image, x1, y1, x2, y2; sampling_ratio 0: the adaptive grid; roi_levels (R) int32
    overrides mmdet's level map; valid (groups) int64: slot r is in use iff r % (R / groups) < valid[r // (R / groups)].
    -> out (R, out_size^2, channels) f32, bin-major and channel-last"""
    R, per = _roi_align_check("roi_align_fwd", rois, roi_levels, valid, out_size, sampling_ratio)
    arr = _roi_levels(maps, sizes, scales, images, channels)
    shape = (R, out_size * out_size, channels)
    out = _scratch(shape, rois.device, torch.float32) if out is None else out
    assert tuple(out.shape) == shape and (levels_out is None or (levels_out.dtype == torch.int32 and tuple(levels_out.shape) == (R,)))
    check(lib().mtp_roi_align_fwd(arr, len(sizes), images, channels, _f32(rois), _p(roi_levels), _p(valid), R, per, out_size, sampling_ratio,
                                  int(bool(aligned)), float(finest_scale), _f32(out), _p(levels_out), _s()), "mtp_roi_align_fwd")
    return out


def roi_align_bwd(dout, dmaps, sizes, scales, channels, images, rois, out_size=14, sampling_ratio=0, aligned=True, finest_scale=56.0, roi_levels=None,
                  valid=None, accumulate=False):
    """the gradient of roi_align_fwd with respect to the maps, deterministic, one launch, no workspace: a gather per map pixel over the RoIs in
    index order.  dout (R, out_size^2, channels); dmaps: per level a triple in the maps' layout.  EVERY pixel is stored, or added to what is
    there when accumulate.  No gradient to the RoIs (mmcv has none)."""
    R, per = _roi_align_check("roi_align_bwd", rois, roi_levels, valid, out_size, sampling_ratio)
    if dout.dtype != torch.float32 or tuple(dout.shape) != (R, out_size * out_size, channels) or not dout.is_contiguous():
        raise TypeError("roi_align_bwd: dout must be contiguous float32 of shape (R, out_size^2, channels)")
    arr = _roi_levels(dmaps, sizes, scales, images, channels, grads=True)
    check(lib().mtp_roi_align_bwd(arr, len(sizes), images, channels, _f32(dout), _f32(rois), _p(roi_levels), _p(valid), R, per, out_size,
                                  sampling_ratio, int(bool(aligned)), float(finest_scale), int(bool(accumulate)), _s()), "mtp_roi_align_bwd")
    return dmaps


def mask_loss(mask_preds, boxes, labels, sample_gt, n_pos, bitmaps, img_hw=None, loss_weight=1.0, dlogits=None, want_avg=False, out=None, num_classes=None):
    """Mask targets and the mask loss of the whole batch (mtp_mask_loss): two launches, no host synchronisation.  mask_preds (images * S, K, M, M)
    f32 logits; boxes (images * S, 4); labels (images * S) int64 the class channel of each slot, or None (class-agnostic: channel 0); sample_gt
    (images, S) int64 rows of bitmaps (G, H, W) uint8; n_pos (images) int64 on the device; img_hw (images, 2) int64 or None.
    dlogits: a buffer like mask_preds for the gradient, every element stored.  num_classes: the labels name the first num_classes of the K
    channels (a GEMM output padded to 8 columns); a slot with a label beyond them is padding.
    -> dict(loss (1), targets (images * S, M, M) uint8, slot_loss (images * S), target_avg (like targets, f32) when want_avg)"""
    if mask_preds.dtype != torch.float32 or mask_preds.dim() != 4 or mask_preds.shape[2] != mask_preds.shape[3] or not mask_preds.is_contiguous():
        raise TypeError("mask_loss: mask_preds must be contiguous float32 of shape (slots, K, M, M)")
    R, K, M, _ = mask_preds.shape
    classes = K if num_classes is None else int(num_classes)
    if not 1 <= classes <= K:
        raise ValueError("mask_loss: num_classes in 1 .. %d, the channels of mask_preds" % K)
    if sample_gt.dim() != 2 or sample_gt.numel() != R or R == 0:
        raise ValueError("mask_loss: sample_gt (images, S) with images * S = %d slots > 0" % R)
    images, S = sample_gt.shape
    _check_boxes("mask_loss", boxes, 4)
    if boxes.shape[0] != R:
        raise ValueError("mask_loss: one box per slot")
    if bitmaps.dtype != torch.uint8 or bitmaps.dim() != 3 or not bitmaps.is_contiguous():
        raise TypeError("mask_loss: bitmaps must be contiguous uint8 of shape (G, H, W)")
    G, H, W = bitmaps.shape
    for t, shape in ((sample_gt, (images, S)), (n_pos, (images,))) + (() if labels is None else ((labels, (R,)),)) + (() if img_hw is None else ((img_hw, (images, 2)),)):
        if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError("mask_loss: sample_gt (images, S), n_pos (images), labels (slots) and img_hw (images, 2) are contiguous int64")
    if dlogits is not None and (dlogits.dtype != torch.float32 or tuple(dlogits.shape) != tuple(mask_preds.shape) or not dlogits.is_contiguous()):
        raise TypeError("mask_loss: dlogits has the layout of mask_preds")
    if H < 1 or W < 1:
        raise ValueError("mask_loss: the bitmaps have at least one pixel")
    dev = mask_preds.device
    if out is None:
        out = dict(loss=_scratch((1,), dev, torch.float32), targets=_scratch((R, M, M), dev, torch.uint8), slot_loss=_scratch((R,), dev, torch.float32))
        if want_avg:
            out["target_avg"] = _scratch((R, M, M), dev, torch.float32)
    avg = out.get("target_avg")
    assert tuple(out["loss"].shape) == (1,) and tuple(out["targets"].shape) == (R, M, M) and out["targets"].dtype == torch.uint8
    assert tuple(out["slot_loss"].shape) == (R,) and (avg is None or tuple(avg.shape) == (R, M, M))
    check(lib().mtp_mask_loss(_f32(mask_preds), classes, K, M, _f32(boxes), _p(labels), _p(sample_gt), _p(n_pos), images, S, _p(bitmaps) if G else None, G, H, W,
                              _p(img_hw), float(loss_weight), _p(out["targets"]), _p(avg), _f32(out["slot_loss"]), _f32(out["loss"]), _p(dlogits), _s()),
          "mtp_mask_loss")
    return out


def mask_paste(mask_preds, labels, boxes, img_h, img_w, threshold=0.5, activate=True, out=None, values=None):
    """_do_paste_mask(skip_empty=False) and the threshold in one launch: mask_preds (N > 0, K, M, M) f32, labels (N) int64 or None (channel 0),
    boxes (N, 4) -> (N, img_h, img_w) bool (threshold >= 0) or uint8 (threshold < 0: value * 255).  values: an (N, img_h, img_w) f32 buffer for
    the sampled values."""
    if mask_preds.dtype != torch.float32 or mask_preds.dim() != 4 or mask_preds.shape[2] != mask_preds.shape[3] or not mask_preds.is_contiguous():
        raise TypeError("mask_paste: mask_preds must be contiguous float32 of shape (N, K, M, M)")
    N, K, M, _ = mask_preds.shape
    _check_boxes("mask_paste", boxes, 4)
    if N == 0 or boxes.shape[0] != N or img_h < 1 or img_w < 1:
        raise ValueError("mask_paste: N > 0 instances with one box each, and an image of at least one pixel")
    if labels is not None and (labels.dtype != torch.int64 or tuple(labels.shape) != (N,) or not labels.is_contiguous()):
        raise TypeError("mask_paste: labels must be contiguous int64 of shape (N,)")
    shape = (N, int(img_h), int(img_w))
    out = _scratch(shape, mask_preds.device, torch.uint8) if out is None else out
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()
    assert values is None or (values.dtype == torch.float32 and tuple(values.shape) == shape and values.is_contiguous())
    check(lib().mtp_mask_paste(_f32(mask_preds), K, M, _p(labels), _f32(boxes), N, shape[1], shape[2], float(threshold), int(bool(activate)), _p(out),
                               _p(values), _s()), "mtp_mask_paste")
    return out.view(torch.bool) if threshold >= 0 else out


# ------------------------------------------------------------------------------------------------ the box half of Mask R-CNN (csrc/hbox_head.hip)
HBOX_DELTAS = 4
HBOX_WH_RATIO_CLIP = 16 / 1000
HROI_TARGET = {"reference": _lib.HROI_TARGET_ONES, "encoded": _lib.HROI_TARGET_ENCODED}


def _hbox_codec(means, stds):
    m, s = [float(v) for v in means], [float(v) for v in stds]
    if len(m) != HBOX_DELTAS or len(s) != HBOX_DELTAS or min(s) <= 0:
        raise ValueError("the delta-xywh coder takes 4 means and 4 positive stds")
    return (C.c_float * 4)(*m), (C.c_float * 4)(*s)


def _hbox_clip(wh_ratio_clip):
    if not wh_ratio_clip > 0:
        raise ValueError("wh_ratio_clip must be positive")
    return float(wh_ratio_clip)


def _hbox_table(name, t, images, what):
    """a per-image (images, 2) f32 table on the device: (h, w) shapes or (1 / sx, 1 / sy) factors"""
    if t.dtype != torch.float32 or tuple(t.shape) != (images, 2) or not t.is_cuda:
        raise TypeError("%s: %s must be a float32 device tensor of shape (images, 2)" % (name, what))
    return _f32(t)


def hbox_delta_encode(priors, gts, means, stds, out=None):
    """DeltaXYWHBBoxCoder encode (mmdet bbox2delta): priors (n, 4), gts (n, 4) -> deltas (n, 4)"""
    _check_boxes("hbox_delta_encode", priors, 4)
    _check_boxes("hbox_delta_encode", gts, 4)
    n = priors.shape[0]
    assert gts.shape[0] == n and n > 0
    out = _scratch((n, 4), priors.device, torch.float32) if out is None else out
    assert tuple(out.shape) == (n, 4)
    m, s = _hbox_codec(means, stds)
    check(lib().mtp_hbox_delta_encode(_f32(priors), _f32(gts), m, s, n, _f32(out), _s()), "mtp_hbox_delta_encode")
    return out


def hbox_delta_decode(priors, deltas, means, stds, max_shapes=None, image_ids=None, wh_ratio_clip=HBOX_WH_RATIO_CLIP, out=None):
    """DeltaXYWHBBoxCoder decode (mmdet delta2bbox): priors (n, 4), deltas (n, 4) -> boxes (n, 4).  max_shapes: None (no clip) or an (images, 2)
    f32 device table of (h, w); image_ids (n) int64: the image of each row (None: image 0).  One launch for the whole batch."""
    _check_boxes("hbox_delta_decode", priors, 4)
    _check_boxes("hbox_delta_decode", deltas, 4)
    n = priors.shape[0]
    assert deltas.shape[0] == n and n > 0
    images = 0
    if max_shapes is None:
        if image_ids is not None:
            raise ValueError("hbox_delta_decode: image_ids without max_shapes")
    else:
        images = max_shapes.shape[0]
        _hbox_table("hbox_delta_decode", max_shapes, images, "max_shapes")
        if image_ids is not None and (image_ids.dtype != torch.int64 or tuple(image_ids.shape) != (n,)):
            raise TypeError("hbox_delta_decode: image_ids must be int64 of shape (n,)")
    out = _scratch((n, 4), priors.device, torch.float32) if out is None else out
    assert tuple(out.shape) == (n, 4)
    m, s = _hbox_codec(means, stds)
    check(lib().mtp_hbox_delta_decode(_f32(priors), _f32(deltas), m, s, _hbox_clip(wh_ratio_clip), n, _f32(max_shapes), _p(image_ids), images, _f32(out),
                                      _s()), "mtp_hbox_delta_decode")
    return out


def hrpn_loss(cls_maps, reg_maps, sizes, A, priors, gts, samples, sample_gt, n_pos, n_neg, means, stds, cls_weight=1.0, bbox_weight=1.0, dcls=None,
              dreg=None, loss_cls=None, loss_bbox=None):
    """Targets and loss of the horizontal RPN for the whole batch (mtp_hrpn_loss): rpn_loss with four deltas per anchor, gts (K, 4) and L1.
    dcls / dreg: gradient maps in the maps' layout, ZEROED by the caller (both or neither).  -> (loss_cls (levels), loss_bbox (levels)) f32"""
    _check_boxes("hrpn_loss", priors, 4)
    _check_boxes("hrpn_loss", gts, 4)
    images, S = samples.shape
    if (dcls is None) != (dreg is None):
        raise ValueError("hrpn_loss: dcls and dreg come together")
    arr, total = _rpn_levels(cls_maps, reg_maps, sizes, A, images, dcls, dreg, deltas=HBOX_DELTAS)
    if priors.shape[0] != total:
        raise ValueError("hrpn_loss: %d priors for %d anchors" % (priors.shape[0], total))
    for t, shape in ((samples, (images, S)), (sample_gt, (images, S)), (n_pos, (images,)), (n_neg, (images,))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape:
            raise TypeError("hrpn_loss: samples, sample_gt (images, S) and n_pos, n_neg (images) are int64")
    dev, n = priors.device, len(sizes)
    loss_cls = _scratch((n,), dev, torch.float32) if loss_cls is None else loss_cls
    loss_bbox = _scratch((n,), dev, torch.float32) if loss_bbox is None else loss_bbox
    assert tuple(loss_cls.shape) == tuple(loss_bbox.shape) == (n,)
    wb = lib().mtp_hrpn_loss_workspace_bytes(images, S)
    ws = _scratch((wb // 4,), dev, torch.float32)
    m, s = _hbox_codec(means, stds)
    K = gts.shape[0]
    check(lib().mtp_hrpn_loss(arr, n, A, _f32(priors), total, _f32(gts) if K else None, K, _p(samples), _p(sample_gt), _p(n_pos), _p(n_neg), images, S, m, s,
                              float(cls_weight), float(bbox_weight), _f32(loss_cls), _f32(loss_bbox), _p(ws), wb, _s()), "mtp_hrpn_loss")
    return loss_cls, loss_bbox


def hrpn_proposals(cls_maps, reg_maps, sizes, A, priors, keep, keep_counts, means, stds, img_shapes, min_bbox_size=0.0,
                   wh_ratio_clip=HBOX_WH_RATIO_CLIP, out=None):
    """keep (images, T) int64 as rpn_proposals takes it; img_shapes (images, 2) f32 (h, w) on the device.
    -> scores (images, T) f32, boxes (images, T, 4) clipped to the image, level_ids (images, T) int64, valid (images, T) uint8.  One launch."""
    _check_boxes("hrpn_proposals", priors, 4)
    images, T = keep.shape
    if keep.dtype != torch.int64 or T != sum(int(k) for k in keep_counts) or T == 0:
        raise TypeError("hrpn_proposals: keep must be int64 of shape (images, sum(keep_counts) > 0)")
    arr, total = _rpn_levels(cls_maps, reg_maps, sizes, A, images, keep_counts=keep_counts, deltas=HBOX_DELTAS)
    if priors.shape[0] != total:
        raise ValueError("hrpn_proposals: %d priors for %d anchors" % (priors.shape[0], total))
    shapes = _hbox_table("hrpn_proposals", img_shapes, images, "img_shapes")
    dev = priors.device
    if out is None:
        out = (_scratch((images, T), dev, torch.float32), _scratch((images, T, 4), dev, torch.float32), _scratch((images, T), dev, torch.int64),
               _scratch((images, T), dev, torch.uint8))
    scores, boxes, level_ids, valid = out
    assert tuple(scores.shape) == tuple(level_ids.shape) == tuple(valid.shape) == (images, T) and level_ids.dtype == torch.int64 and valid.dtype == torch.uint8
    assert tuple(boxes.shape) == (images, T, 4)
    m, s = _hbox_codec(means, stds)
    check(lib().mtp_hrpn_proposals(arr, len(sizes), A, _f32(priors), total, _p(keep), images, m, s, _hbox_clip(wh_ratio_clip), shapes, float(min_bbox_size),
                                   _f32(scores), _f32(boxes), _p(level_ids), _p(valid), _s()), "mtp_hrpn_proposals")
    return scores, boxes, level_ids, valid


def _hroi_reg_rows(name, t, num_classes):
    """(rows, >= 4 K) f32 rows whose pitch is a multiple of 4 elements and whose base is 16-byte aligned: class k is one 16-byte access"""
    ptr, ld = _roi_rows(name, t, 4 * num_classes)
    if ld % 4 or ptr % 16:
        raise ValueError("%s: the 4 K deltas of a row start on 16 bytes (pitch a multiple of 4 floats)" % name)
    return ptr, ld


def hroi_loss(cls_score, bbox_pred, num_classes, rois, gts, gt_labels, sample_gt, n_pos, n_neg, means, stds, reg_target="reference", cls_weight=1.0,
              bbox_weight=1.0, dcls=None, dreg=None, losses=None):
    """Targets and losses of the per-class bbox head for the whole batch (mtp_hroi_loss): two launches, no host synchronisation.  cls_score (images *
    S, num_classes + 1) and bbox_pred (images * S, 4 * num_classes): rows of a wider buffer are fine; rois (images * S, 4); gts (G, 4), gt_labels (G);
    sample_gt (images, S), n_pos, n_neg (images) int64.  reg_target: 'reference' (all ones, instance_segmentation/base_bbox_head.py as written) or
    'encoded' (mmdet: encode(roi, gt)).  dcls / dreg: the gradients in the layout of their inputs, dreg dense: every class column of every row is
    stored.  -> losses (3) f32: loss_cls, loss_bbox, acc in percent"""
    images, S = sample_gt.shape
    R = images * S
    _check_boxes("hroi_loss", rois, 4)
    _check_boxes("hroi_loss", gts, 4)
    if reg_target not in HROI_TARGET:
        raise ValueError("hroi_loss: reg_target is 'reference' or 'encoded', got %r" % (reg_target,))
    if R == 0 or rois.shape[0] != R or cls_score.shape[0] != R or bbox_pred.shape[0] != R:
        raise ValueError("hroi_loss: %d rows for %d x %d slots" % (rois.shape[0], images, S))
    G = gts.shape[0]
    for t, shape in ((sample_gt, (images, S)), (n_pos, (images,)), (n_neg, (images,)), (gt_labels, (G,))):
        if t.dtype != torch.int64 or tuple(t.shape) != shape:
            raise TypeError("hroi_loss: sample_gt (images, S), n_pos, n_neg (images) and gt_labels (G) are int64")
    (pc, ldc), (pr, ldr) = _roi_rows("hroi_loss", cls_score, num_classes + 1), _hroi_reg_rows("hroi_loss", bbox_pred, num_classes)
    if (dcls is None) != (dreg is None):
        raise ValueError("hroi_loss: dcls and dreg come together")
    pdc = pdr = None
    if dcls is not None:
        (pdc, a), (pdr, b) = _roi_rows("hroi_loss", dcls, num_classes + 1), _hroi_reg_rows("hroi_loss", dreg, num_classes)
        if a != ldc or b != ldr or dcls.shape[0] != R or dreg.shape[0] != R:
            raise ValueError("hroi_loss: a gradient has the layout of its input")
    dev = rois.device
    losses = _scratch((3,), dev, torch.float32) if losses is None else losses
    assert tuple(losses.shape) == (3,)
    wb = lib().mtp_hroi_loss_workspace_bytes(images, S)
    ws = _scratch((wb // 4,), dev, torch.float32)
    m, s = _hbox_codec(means, stds)
    check(lib().mtp_hroi_loss(pc, ldc, pr, ldr, int(num_classes), _f32(rois), _f32(gts) if G else None, _p(gt_labels) if G else None, G, _p(sample_gt),
                              _p(n_pos), _p(n_neg), images, S, m, s, HROI_TARGET[reg_target], float(cls_weight), float(bbox_weight), _f32(losses), pdc, pdr,
                              _p(ws), wb, _s()), "mtp_hroi_loss")
    return losses


def hroi_predict(cls_score, bbox_pred, num_classes, rois, means, stds, img_shapes, inv_scale=None, score_thr=0.0, wh_ratio_clip=HBOX_WH_RATIO_CLIP,
                 out=None):
    """rois (R, 5): image, x1, y1, x2, y2.  Per RoI the softmax scores (R, num_classes), the num_classes decoded boxes (R, num_classes, 4) clipped to
    img_shapes[image] (images, 2) f32 (h, w) and multiplied by inv_scale[image] (images, 2) f32 (1 / sx, 1 / sy) when given, and the score >
    score_thr flags (R, num_classes) uint8: one launch"""
    _check_boxes("hroi_predict", rois, 5)
    R = rois.shape[0]
    if R == 0 or cls_score.shape[0] != R or bbox_pred.shape[0] != R:
        raise ValueError("hroi_predict: R > 0 rows of scores, deltas and rois")
    (pc, ldc), (pr, ldr) = _roi_rows("hroi_predict", cls_score, num_classes + 1), _hroi_reg_rows("hroi_predict", bbox_pred, num_classes)
    images = img_shapes.shape[0]
    shapes = _hbox_table("hroi_predict", img_shapes, images, "img_shapes")
    inv = None if inv_scale is None else _hbox_table("hroi_predict", inv_scale, images, "inv_scale")
    dev = rois.device
    if out is None:
        out = (_scratch((R, num_classes), dev, torch.float32), _scratch((R, num_classes, 4), dev, torch.float32), _scratch((R, num_classes), dev, torch.uint8))
    scores, boxes, flags = out
    assert tuple(scores.shape) == tuple(flags.shape) == (R, num_classes) and tuple(boxes.shape) == (R, num_classes, 4) and flags.dtype == torch.uint8
    m, s = _hbox_codec(means, stds)
    check(lib().mtp_hroi_predict(pc, ldc, pr, ldr, int(num_classes), _f32(rois), R, m, s, _hbox_clip(wh_ratio_clip), shapes, inv, images, float(score_thr),
                                 _f32(scores), _f32(boxes), _p(flags), _s()), "mtp_hroi_predict")
    return scores, boxes, flags
