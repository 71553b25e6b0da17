"""The classification head's four launches (mtp_gap_fwd, mtp_cls_ce, mtp_cls_head_bwd, mtp_gap_bwd) against the torch-operator composition on the
same GPU (adaptive_avg_pool2d -> F.linear -> F.cross_entropy and its autograd), at ViT-L's scene-classification shape by default: N 64, C 1024,
HW 196, K 45, bf16 maps.  Device-event pairs around one forward + backward of each, the two alternating in one process after a warm-up; medians, the
spread (min, max) and the HBM floor of the two map-sized passes.  One JSON line.  Not a test.
Usage: python tools/cls_head_probe.py [--n 64 --c 1024 --hw 14 --k 45 --iters 200 --warmup 20 --dtype bf16]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtp_amd import ops  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--c", type=int, default=1024)
    ap.add_argument("--hw", type=int, default=14, help="side of the square map")
    ap.add_argument("--k", type=int, default=45)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.n, a.c, a.hw, a.hw, generator=g).to(dt).cuda()
    w, b = torch.randn(a.k, a.c, generator=g).mul_(0.01).cuda(), torch.zeros(a.k).cuda()
    labels = torch.randint(0, a.k, (a.n,), generator=g).cuda()
    dw, db, dp, dx = torch.zeros_like(w), torch.zeros_like(b), torch.empty(a.n, a.c, device="cuda"), torch.empty_like(x)
    xt, wt, bt = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def fused():
        pooled = ops.gap_fwd(x)
        out = ops.cls_ce(pooled, w, b, labels, 1.0, check_labels=False)
        ops.cls_head_bwd(out["dlogits"], pooled, w, dw, db, dp, accumulate=True)
        ops.gap_bwd(dp, dx)
        return out["loss"]

    def composed():
        xt.grad = None
        loss = F.cross_entropy(F.linear(F.adaptive_avg_pool2d(xt, 1).flatten(1).float(), wt, bt), labels)
        loss.backward()      # (accumulates into wt.grad / bt.grad, as the fused path does into dw / db)
        return loss

    for _ in range(a.warmup):
        lf, lc = fused(), composed()
    torch.cuda.synchronize()
    agree = abs(float(lf) - float(lc)) / float(lc)
    times = {"fused": [], "composed": []}
    for i in range(a.iters):
        for name, fn in ((("fused", fused), ("composed", composed)) if i % 2 == 0 else (("composed", composed), ("fused", fused))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    map_bytes = x.numel() * x.element_size()
    res = {"shape": dict(N=a.n, C=a.c, HW=a.hw * a.hw, K=a.k, dtype=a.dtype), "iters": a.iters, "loss_rel_diff": agree,
           "map_bytes_each_way": map_bytes, "hbm_floor_us_each_way": map_bytes / PEAK * 1e6}
    for name, t in times.items():
        res[name + "_us"] = dict(median=statistics.median(t), min=min(t), max=max(t))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
