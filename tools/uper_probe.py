"""UperNet decode head in the training step: one DataParallelTrainer step (backbone fwd + head fwd + fused loss + head bwd + backbone bwd + clip + AdamW)
with the head against the same step with a plain stand-in loss, per case, bf16:
  vitl     -- ViT-L + RVSA 224^2, B = 64 in slices of 22 / 21 / 21 (slice_classes 8 / 8 / 8), channels 256 (the MTP pretraining arrangement)
  xl       -- InternImage-XL 512^2, B = 8, channels 512, 7 classes
  vitl512  -- ViT-L + RVSA 512^2, B = 1, channels 512, 7 classes: next to the reference's 1.538 s/iter (BASELINE.md:37)
and, at each case's largest head map, the achieved HBM rate of the BN (two statistics passes + apply), resize and loss kernels on their algorithmic
bytes, as a fraction of 8 TB/s.  One JSON line per case.  Usage: python tools/uper_probe.py [--cases vitl,xl,vitl512] [--iters 5]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtp_amd  # noqa: E402
from mtp_amd import ops  # noqa: E402
from mtp_amd.parallel import DataParallelTrainer  # noqa: E402

PEAK = 8.0e12
CASES = {
    "vitl": dict(model="vit_l", img=224, B=64, channels=256, classes=(8, 8, 8), slices=(22, 21, 21)),
    "xl": dict(model="internimage_xl", img=512, B=8, channels=512, classes=7, slices=None),
    "vitl512": dict(model="vit_l", img=512, B=1, channels=512, classes=7, slices=None),
}


def _net(c):
    torch.manual_seed(2023)
    if c["model"] == "internimage_xl":
        net = mtp_amd.internimage_xl(precision="bf16", with_cp=False)
    else:
        class A:
            image_size = c["img"]
            use_ckpt = "False"
            precision = "bf16"
        net = mtp_amd.vit_l_rvsa(A)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if "rel_pos" in n or ".dcn.offset.weight" in n or ".dcn.mask.weight" in n:
                p.normal_(0, 0.02)
    return net.cuda().train()


def _plain(feats):
    return sum(f.float().mean() for f in feats), [torch.full_like(f, 1.0 / f.numel()) for f in feats]


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def _hbm(N, H, W, C, K, iters):
    """the head's largest map (N*H*W, C) bf16: BN statistics (two passes) + apply, the x2 resize into it, the fused loss at 4x the size"""
    rows = N * H * W
    x = torch.randn(rows, C, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    g, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    mean, rstd, ctr = (torch.empty(C, device="cuda") for _ in range(3))

    def bn():
        ops.bn_finalize(ops.bn_sums(x), rows, None, None, ctr, rstd)
        ops.bn_finalize(ops.bn_sums(x, ctr), rows, None, None, mean, rstd, center=ctr)
        ops.bn_apply(x, mean, rstd, g, b, y)
    src = torch.randn(N * (H // 2) * (W // 2), C, device="cuda").to(torch.bfloat16)

    def rs():
        ops.resize_bilinear_fwd(src, y, N, H // 2, W // 2, H, W, accumulate=True)
    Kp = ops.pad8(K)
    lg = torch.randn(rows, Kp, device="cuda")
    lab = torch.randint(0, K, (N, 4 * H, 4 * W), device="cuda", dtype=torch.uint8)

    def ce():
        ops.seg_ce(lg, K, N, H, W, lab)
    out = {}
    for name, fn, byts in (("bn", bn, rows * C * 2 * 4), ("resize", rs, src.numel() * 2 + 2 * rows * C * 2),
                           ("loss", ce, rows * Kp * 4 + lab.numel() * (1 + 2 * 4 * K) + rows * Kp * 4)):
        ms = _time(fn, iters, 2)
        out[name] = dict(us=round(ms * 1e3, 1), hbm_frac=round(byts / (ms * 1e-3) / PEAK, 3))
    return out


def run(name, c, iters, warmup):
    net = _net(c)
    img = torch.randn(c["B"], 3, c["img"], c["img"], device="cuda")
    tr = DataParallelTrainer(net, lr=6e-5, weight_decay=0.05, max_norm=5.0, total_steps=1000, feature_dtype=torch.bfloat16)
    base = _time(lambda: tr.step(img, _plain), iters, warmup)
    del tr
    chans = list(net.out_channels) if hasattr(net, "out_channels") else [net.embed_dim] * 4
    kw = dict(in_channels=chans, channels=c["channels"], precision="bf16")
    kw.update(dict(num_classes=1, slice_classes=c["classes"]) if c["slices"] else dict(num_classes=c["classes"]))
    head = mtp_amd.UPerHead(**kw).cuda().train()
    tr = DataParallelTrainer(net, lr=6e-5, weight_decay=0.05, max_norm=5.0, total_steps=1000, feature_dtype=torch.bfloat16, decode_head=head)
    K = max(c["classes"]) if c["slices"] else c["classes"]
    labels = torch.randint(0, K if not c["slices"] else min(c["classes"]), (c["B"], c["img"], c["img"]), device="cuda", dtype=torch.uint8)
    fn = head.loss_and_grads(labels, slices=c["slices"])
    with_head = _time(lambda: tr.step(img, fn), iters, warmup)
    H0 = c["img"] // 4
    res = dict(case=name, batch=c["B"], step_ms_without_head=round(base, 2), step_ms_with_head=round(with_head, 2),
               head_share=round((with_head - base) / with_head, 3), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
               kernels_at_largest_map=_hbm(c["B"], H0, H0, c["channels"], K, iters))
    if name == "vitl512":
        res["reference_s_per_iter"] = 1.538
    del tr, head, net
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="vitl,xl,vitl512")
    a = ap.parse_args()
    for n in a.cases.split(","):
        print(json.dumps(run(n, CASES[n], a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
