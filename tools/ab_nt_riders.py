"""A/B of the NT GEMM riders on the two ViT-L launches that carry them (B = 64: 12544 tokens, 256 windows):
  forward   qkv GEMM 12544 x 3072 x 1024 (persistent, 672 tiles)   with / without rvsa_sampling_fwd
  backward  qkv data gradient 12544 x 1024 x 3072 (one round, 224 tiles) with / without rvsa_sampling_bwd_win
Per launch group, timed with device events around EVERY launch, variants interleaved round by round in one process, operands rotated over 4 buffers:
  gemm        mtp_gemm_nt alone (one workgroup per CU)
  even        the GEMM alone on the workgroups it has under riders (224 of 256): what giving up the uneven walk costs
  gemm+kernel the GEMM and the stand-alone kernel back to back (what the step ran before)
  riding      one launch, the operator on the CUs the GEMM leaves idle
The riding launch counts as a gain only if it is shorter than gemm+kernel by more than the launch-to-launch spread (standard deviation) of `gemm`.
usage: python tools/ab_nt_riders.py [rounds] [launches per round]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from mtp_amd import _lib, ops

T, C, H, B, HP = 12544, 1024, 16, 64, 14
BF, F32 = torch.bfloat16, torch.float32
ROT = 4


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s, dt=F32, sc=1.0: (torch.randn(*s, device="cuda", generator=g) * sc).to(dt)
    nh, nw = ops.rvsa_windows(HP, HP)
    R, N = B * nh * nw, 5 * H
    ln1 = [rn(T, C, dt=BF) for _ in range(ROT)]
    dqkv = [rn(T, 3 * C, dt=BF) for _ in range(ROT)]
    wqkv, wqkvT, bqkv = rn(3 * C, C, dt=BF, sc=0.02), rn(C, 3 * C, dt=BF, sc=0.02), rn(3 * C)
    ws, bs = rn(N, C, sc=0.05), rn(N)
    qkv = [torch.empty(T, 3 * C, device="cuda", dtype=BF) for _ in range(ROT)]
    dln1 = [torch.empty(T, C, device="cuda", dtype=BF) for _ in range(ROT)]
    avg, pooled = [torch.empty(R, C, device="cuda") for _ in range(ROT)], [torch.empty(R, C, device="cuda") for _ in range(ROT)]
    samp, gw = [torch.empty(R, N, device="cuda") for _ in range(ROT)], [torch.empty(R, C, device="cuda") for _ in range(ROT)]
    dsamp, avg_in = rn(R, N), rn(R, C)
    none = _lib.NtRider(kind=_lib.NT_RIDER_NONE)

    def fwd(kind, i):
        k = i % ROT
        if kind == "gemm":
            ops.gemm_nt(ln1[k], wqkv, qkv[k], bias=bqkv)
        elif kind == "even":
            ops.gemm_nt(ln1[k], wqkv, qkv[k], bias=bqkv, rider=none)
        elif kind == "gemm+kernel":
            ops.rvsa_sampling_fwd(ln1[k], ws, bs, avg[k], pooled[k], samp[k], B, HP, HP)
            ops.gemm_nt(ln1[k], wqkv, qkv[k], bias=bqkv)
        elif kind == "kernel":
            ops.rvsa_sampling_fwd(ln1[k], ws, bs, avg[k], pooled[k], samp[k], B, HP, HP)
        else:
            ops.gemm_nt(ln1[k], wqkv, qkv[k], bias=bqkv, rider=ops.sampling_fwd_rider(ln1[k], ws, bs, avg[k], pooled[k], samp[k], B, HP, HP))

    def bwd(kind, i):
        k = i % ROT
        if kind == "gemm":
            ops.gemm_nt(dqkv[k], wqkvT, dln1[k])
        elif kind == "even":
            ops.gemm_nt(dqkv[k], wqkvT, dln1[k], rider=none)
        elif kind == "gemm+kernel":
            ops.rvsa_sampling_bwd_win(dsamp, ws, avg_in, gw[k])
            ops.gemm_nt(dqkv[k], wqkvT, dln1[k])
        elif kind == "kernel":
            ops.rvsa_sampling_bwd_win(dsamp, ws, avg_in, gw[k])
        else:
            ops.gemm_nt(dqkv[k], wqkvT, dln1[k], rider=ops.sampling_bwd_win_rider(dsamp, ws, avg_in, gw[k]))

    kinds = ("gemm", "even", "kernel", "gemm+kernel", "riding")
    for name, fn in (("forward  qkv 12544 x 3072 x 1024 + rvsa_sampling_fwd", fwd), ("backward dqkv 12544 x 1024 x 3072 + rvsa_sampling_bwd_win", bwd)):
        # the riding launch against the two launches it replaces, bit for bit, before anything is timed
        fn("gemm+kernel", 0)
        ref = [t[0].clone() for t in ((qkv, avg, pooled, samp) if fn is fwd else (dln1, gw))]
        for t in ((qkv, avg, pooled, samp) if fn is fwd else (dln1, gw)):
            t[0].fill_(float("nan"))
        fn("riding", 0)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b[0]) for a, b in zip(ref, (qkv, avg, pooled, samp) if fn is fwd else (dln1, gw)))
        for kind in kinds:      # warm-up: code objects, LDS opt-in
            for i in range(4):
                fn(kind, i)
        torch.cuda.synchronize()
        ev = {k: [] for k in kinds}
        for _ in range(rounds):
            for kind in kinds:
                ev[kind] += [timed(lambda: fn(kind, i)) for i in range(per)]
            torch.cuda.synchronize()
        us = {k: [s.elapsed_time(e) * 1e3 for s, e in v] for k, v in ev.items()}
        print("%s   (bit-identical: %s; %d launches per variant)" % (name, same, rounds * per))
        for kind in kinds:
            v = us[kind]
            print("  %-12s median %7.2f us   mean %7.2f   stdev %5.2f   min %7.2f   max %7.2f" % (kind, statistics.median(v), statistics.mean(v), statistics.pstdev(v), min(v), max(v)))
        gain = statistics.median(us["gemm+kernel"]) - statistics.median(us["riding"])
        spread = statistics.pstdev(us["gemm"])
        print("  riding saves %.2f us per launch against gemm+kernel; spread of gemm %.2f us -> %s" % (gain, spread, "KEEP" if gain > spread else "DROP"))
        print("  even walk against one workgroup per CU: %+.2f us" % (statistics.median(us["even"]) - statistics.median(us["gemm"])))


if __name__ == "__main__":
    main()
