"""The mask branch on one GPU at the workload's shape (mask_rcnn.py at bench.py's ViT-L configuration): batch 64 of 224 x 224 images, maps of 256 channels
at strides 4 / 8 / 16 / 32, 128 positives per image (8192 RoIs), RoIAlign 14 -> mask 28, 15 classes, 8 ground truths per image; the paste: 100
instances on one 224 x 224 image.  Device-event pairs around each of the four entry points of csrc/mask_head.hip and around the whole
MTP_IS_StandardRoIHead.loss_and_grads ('bf16' and 'fp32'), after warm-ups: median, min and max.  For the four kernels the bytes the algorithm has to
move (computed from the shapes: every map or gradient map once, every output once, dout / the class channel of the logits once) over the median give
the achieved bytes/s and its share of the 8 TB/s HBM peak.  Not a test; no ratio is asked of it.
Usage: python tools/mask_branch_probe.py [--batch 64 --iters 10 --warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mtp_amd import MODELS, ops  # noqa: E402

IMG, STRIDES, C, S, OUT, M, K, GTS, PEAK = 224, (4, 8, 16, 32), 256, 128, 14, 28, 15, 8, 8e12


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def with_rate(t, nbytes):
    rate = nbytes / (t["median_ms"] * 1e-3)
    return dict(t, bytes=int(nbytes), achieved_GBps=rate / 1e9, share_of_8TBps=rate / PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    B, R = a.batch, a.batch * S
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    dev = "cuda"
    feats = [torch.randn(B, C, IMG // s, IMG // s, device=dev) for s in STRIDES]
    size = np.exp(rng.uniform(np.log(8), np.log(200), (R, 2)))
    ctr = rng.uniform(0, IMG, (R, 2))
    boxes = torch.as_tensor(np.concatenate([ctr - size / 2, ctr + size / 2], 1).astype(np.float32), device=dev)
    yy, xx = np.mgrid[0:IMG, 0:IMG]
    bm = np.zeros((B * GTS, IMG, IMG), np.uint8)
    for g in range(B * GTS):
        cy, cx, ry, rx = rng.uniform(40, 184), rng.uniform(40, 184), rng.uniform(8, 60), rng.uniform(8, 60)
        bm[g] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    bitmaps = torch.as_tensor(bm, device=dev)
    sample_gt = torch.as_tensor((np.arange(B)[:, None] * GTS + rng.integers(0, GTS, (B, S))).astype(np.int64), device=dev)
    labels = torch.as_tensor(rng.integers(0, K, R).astype(np.int64), device=dev)
    n_pos = torch.full((B,), S, device=dev, dtype=torch.int64)
    image = torch.arange(B, device=dev, dtype=torch.float32).repeat_interleave(S)[:, None]
    rois = torch.cat([image, boxes], 1).contiguous()
    res = dict(shape=dict(batch=B, image=IMG, strides=STRIDES, channels=C, positives_per_image=S, rois=R, roi_align=OUT, mask=M, classes=K,
                          gts_per_image=GTS), iters=a.iters, warmup=a.warmup)

    rows = [f.permute(0, 2, 3, 1).reshape(-1, C).contiguous() for f in feats]
    sizes = [(IMG // s, IMG // s) for s in STRIDES]
    maps = [ops.rpn_map_rows(r, H, W) for r, (H, W) in zip(rows, sizes)]
    scales = [1.0 / s for s in STRIDES]
    map_bytes = sum(r.numel() for r in rows) * 4
    out = torch.empty(R, OUT * OUT, C, device=dev)
    lv = torch.empty(R, device=dev, dtype=torch.int32)
    res["roi_align_fwd"] = with_rate(timed(lambda: ops.roi_align_fwd(maps, sizes, scales, C, B, rois, OUT, 0, True, 56.0, valid=n_pos, out=out, levels_out=lv),
                                           a.iters, a.warmup), map_bytes + out.numel() * 4)
    res["rois_per_level"] = torch.bincount(lv.long().clamp(min=0), minlength=len(STRIDES)).tolist()
    dout = torch.randn_like(out)
    drows = [torch.empty_like(r) for r in rows]
    dmaps = [(d,) + m[1:] for d, m in zip(drows, maps)]
    res["roi_align_bwd"] = with_rate(timed(lambda: ops.roi_align_bwd(dout, dmaps, sizes, scales, C, B, rois, OUT, 0, True, 56.0, roi_levels=lv, valid=n_pos),
                                           a.iters, a.warmup), map_bytes + dout.numel() * 4)
    del out, dout, drows, dmaps
    logits = torch.randn(R, K, M, M, device=dev)
    dl = torch.empty_like(logits)
    bufs = dict(loss=torch.empty(1, device=dev), targets=torch.empty(R, M, M, device=dev, dtype=torch.uint8), slot_loss=torch.empty(R, device=dev))
    res["mask_loss"] = with_rate(timed(lambda: ops.mask_loss(logits, boxes, labels, sample_gt, n_pos, bitmaps, dlogits=dl, out=bufs), a.iters, a.warmup),
                                 R * M * M * 4 + dl.numel() * 4 + R * M * M + bitmaps.numel())
    res["mask_loss"]["loss"] = float(bufs["loss"][0])
    del logits, dl
    N = 100
    pl, pb = torch.randn(N, K, M, M, device=dev), boxes[:N].clamp(0, IMG).contiguous()
    po = torch.empty(N, IMG, IMG, device=dev, dtype=torch.uint8)
    res["mask_paste_100_instances"] = with_rate(timed(lambda: ops.mask_paste(pl, labels[:N].contiguous(), pb, IMG, IMG, 0.5, out=po), a.iters, a.warmup),
                                                po.numel() + N * M * M * 4)
    conv_logits = torch.nn.Conv2d(C, K, 1).to(dev)
    samples, gt = dict(boxes=boxes, sample_gt=sample_gt, labels=labels, n_pos=n_pos), dict(bitmaps=bitmaps)
    for precision in ("bf16", "fp32"):
        head = MODELS.build(dict(
            type="MTP_IS_StandardRoIHead",
            mask_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=OUT, sampling_ratio=0), out_channels=C,
                                    featmap_strides=list(STRIDES)),
            mask_head=dict(type="MTP_IS_FCNMaskHead", num_convs=4, in_channels=C, conv_out_channels=C, precision=precision),
            train_cfg=dict(mask_size=M, sampler=dict(type="RandomSampler", num=4 * S, pos_fraction=0.25), pos_weight=-1, debug=False))).to(dev)
        res["loss_and_grads_" + precision] = timed(lambda: head.loss_and_grads(feats, samples, gt, conv_logits), max(3, a.iters // 2), a.warmup)
        res["loss_and_grads_" + precision]["loss_mask"] = float(head.loss(feats, samples, gt, conv_logits)["loss_mask"])
        del head
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
