"""Change detection in the training step: one DataParallelTrainer step on the 2N-batch cat([img_from, img_to]) (backbone fwd + pair fusion + UNetHead fwd +
fused loss + head bwd + backbone bwd + clip + AdamW) against the same step with a plain stand-in loss, per case, bf16, 4 pairs of 256^2 images:
  vitl -- ViT-L + RVSA (open-cd body, taps): four 1024-channel 16x16 maps, decoder 512/256/128/64 (the rvsa-l-unet-256 configs)
  xl   -- InternImage-XL: 192/384/768/1536 channels at 64/32/16/8, decoder 512/256/128/64 (the intern-xl-unet-256 configs)
and, at each case's largest block input, mtp_unet_up_cat_fwd and mtp_fuse_pair_fwd on their algorithmic bytes as a fraction of 8 TB/s, next to the
torch expressions they replace timed in the same process (F.interpolate nearest + bilinear + cat on NCHW; two layout changes + sub().abs()):
medians of alternating device-event timings.  One JSON line per case.  Usage: python tools/unet_probe.py [--cases vitl,xl] [--iters 5]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtp_amd  # noqa: E402
from mtp_amd import ops  # noqa: E402
from mtp_amd.parallel import DataParallelTrainer  # noqa: E402

PEAK = 8.0e12
BF16 = torch.bfloat16
CASES = {
    "vitl": dict(model="vit_l", img=256, pairs=4, chans=[1024] * 4, grids=[16, 16, 16, 16]),
    "xl": dict(model="internimage_xl", img=256, pairs=4, chans=[192, 384, 768, 1536], grids=[64, 32, 16, 8]),
}
DECODER = [512, 256, 128, 64]


def _net(c):
    torch.manual_seed(2023)
    if c["model"] == "internimage_xl":
        net = mtp_amd.internimage_xl(precision="bf16", with_cp=False)
    else:
        net = mtp_amd.RVSA_MTP_taps(img_size=c["img"], patch_size=16, drop_path_rate=0.3, out_indices=[7, 11, 15, 23], embed_dim=1024, depth=24, num_heads=16,
                                    mlp_ratio=4, qkv_bias=True, use_abs_pos_emb=True, interval=6, precision="bf16")
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


def _alternate(fa, fb, iters):
    """medians of fa and fb timed in turns (a, b, a, b, ...) after two warm-up rounds"""
    for _ in range(2):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(iters):
        for fn, acc in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            acc.append(a.elapsed_time(b))
    ta.sort()
    tb.sort()
    return ta[len(ta) // 2], tb[len(tb) // 2]


def _kernels(c, iters):
    """the largest block input: the last block that has a skip (block 2: x = decoder[1] channels, the finest encoder map as its skip) and the pair
    fusion of the largest encoder map"""
    N = c["pairs"]
    head_grid = c["grids"][-1]
    h = head_grid << 2                                   # block 2's input grid
    Cx, Cs, hs = DECODER[1], c["chans"][0], c["grids"][0]
    x = torch.randn(N * h * h, Cx, device="cuda").to(BF16)
    sk = torch.randn(N * hs * hs, Cs, device="cuda").to(BF16)
    y = torch.empty(4 * N * h * h, Cx + Cs, device="cuda", dtype=BF16)
    xn, sn = x.view(N, h, h, Cx).permute(0, 3, 1, 2).contiguous(), sk.view(N, hs, hs, Cs).permute(0, 3, 1, 2).contiguous()

    def ours():
        ops.unet_up_cat_fwd(x, sk, y, N, h, h, hs, hs)

    def ref():
        return torch.cat([F.interpolate(xn, scale_factor=2, mode="nearest"), F.interpolate(sn, size=(2 * h, 2 * h), mode="bilinear")], 1)
    a, b = _alternate(ours, ref, iters)
    byts = (x.numel() + sk.numel() + y.numel()) * 2
    out = {"up_cat_fwd": dict(shape="x %dx%dx%d + skip %dx%dx%d -> %dx%dx%d" % (h, h, Cx, hs, hs, Cs, 2 * h, 2 * h, Cx + Cs), us=round(a * 1e3, 1),
                              hbm_frac=round(byts / (a * 1e-3) / PEAK, 3), torch_us=round(b * 1e3, 1))}
    Cf, g = c["chans"][0], c["grids"][0]
    f = torch.randn(2 * N, Cf, g, g, device="cuda").to(BF16)
    rows = torch.empty(N * g * g, Cf, device="cuda", dtype=BF16)

    def ours2():
        ops.fuse_pair_fwd(f, rows, "abs_diff")

    def ref2():
        return (f[:N].permute(0, 2, 3, 1).contiguous() - f[N:].permute(0, 2, 3, 1).contiguous()).abs()
    a, b = _alternate(ours2, ref2, iters)
    byts = (f.numel() + rows.numel()) * 2
    out["fuse_pair_fwd"] = dict(shape="%dx%dx%dx%d" % (2 * N, Cf, g, g), us=round(a * 1e3, 1), hbm_frac=round(byts / (a * 1e-3) / PEAK, 3), torch_us=round(b * 1e3, 1))
    return out


def run(name, c, iters, warmup):
    net = _net(c)
    N = c["pairs"]
    img = torch.randn(2 * N, 3, c["img"], c["img"], device="cuda")
    tr = DataParallelTrainer(net, lr=6e-5, weight_decay=0.05, max_norm=5.0, total_steps=1000, feature_dtype=BF16)
    base = _time(lambda: tr.step(img, _plain), iters, warmup)
    del tr
    head = mtp_amd.UNetHead(encoder_channels=c["chans"], decoder_channels=DECODER, n_blocks=4, num_classes=2, precision="bf16").cuda().train()
    tr = DataParallelTrainer(net, lr=6e-5, weight_decay=0.05, max_norm=5.0, total_steps=1000, feature_dtype=BF16, decode_head=head)
    labels = torch.randint(0, 2, (N, c["img"], c["img"]), device="cuda", dtype=torch.uint8)
    fn = head.loss_and_grads(labels, fusion="abs_diff")
    with_head = _time(lambda: tr.step(img, fn), iters, warmup)
    res = dict(case=name, pairs=N, step_ms_without_head=round(base, 2), step_ms_with_head=round(with_head, 2),
               head_share=round((with_head - base) / with_head, 3), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
               kernels_at_largest_block=_kernels(c, max(iters, 10)))
    del tr, head, net
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="vitl,xl")
    a = ap.parse_args()
    for n in a.cases.split(","):
        print(json.dumps(run(n, CASES[n], a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
