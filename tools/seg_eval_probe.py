"""Sliding-window evaluation after the backbone: one 1024^2 image, 7 classes, nine 512^2 windows at stride 384 ((1024 - 512 + 383) // 384 + 1 = 3 per side,
the last clamped to origin 512), UPerHead(channels 512) on ViT-L-sized features (1024 channels, maps 128 / 64 / 32 / 16 per window), bf16.
  new  -- EncoderDecoder.predict(metric=IoUMetric, labels=...) behind a stand-in backbone that returns fixed features: head rows -> window accumulate ->
          arg-max + areas (csrc/seg_eval.hip), and compute_metrics' one sync
  old  -- what a caller had to write before: UPerHead.predict per window (pad, rows, resize, NCHW), preds += F.pad(...), count_mat, the division,
          torch.argmax, three masked torch.histc and a .cpu() (the reference metric's steps); UPerHead.predict is unchanged, so this also times the parent
and the evaluation passes alone on precomputed per-window logits (`eval_only_*`).  The two are timed alternately in one process; medians of device-event
times.  One JSON line.  Run by hand: python tools/seg_eval_probe.py [--iters 10]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mtp_amd  # noqa: E402
from mtp_amd import ops  # noqa: E402
from mtp_amd.segmentors.encoder_decoder import slide_origins, window_counts  # noqa: E402

IMG, CROP, STRIDE, K, C = 1024, 512, 384, 7, 1024


class FixedFeatures(torch.nn.Module):
    """stand-in backbone: the same four maps for every window (the probe times what comes after the backbone)"""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, x):
        return self.feats


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _areas_torch(pred, lab, ignore=255):
    """metric.py's steps: mask, three histc, .cpu()"""
    mask = lab != ignore
    p, l = pred[mask], lab[mask]
    hs = [torch.histc(t.float(), bins=K, min=0, max=K - 1).cpu() for t in (p[p == l], p, l)]
    return hs[0], hs[1] + hs[2] - hs[0], hs[1], hs[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = "cuda"
    feats = [torch.randn(1, C, CROP // s, CROP // s, device=dev).to(torch.bfloat16) for s in (4, 8, 16, 32)]
    head = mtp_amd.UPerHead(in_channels=[C] * 4, channels=512, num_classes=K, precision="bf16").to(dev).eval()
    with torch.no_grad():
        head.conv_seg.weight.normal_(0.0, 1.0)
    model = mtp_amd.EncoderDecoder(FixedFeatures(feats), head, test_cfg=dict(mode="slide", crop_size=(CROP, CROP), stride=(STRIDE, STRIDE))).eval()
    img = torch.zeros(1, 3, IMG, IMG, device=dev)
    lab = torch.randint(0, K, (1, IMG, IMG), device=dev, dtype=torch.uint8)
    origins = slide_origins(IMG, CROP, STRIDE)
    assert origins == [0, 384, 512]
    wins = [(y, x) for y in origins for x in origins]

    def new():
        m = mtp_amd.IoUMetric(K)
        model.predict(img, metric=m, labels=lab)
        return m.compute_metrics()

    @torch.no_grad()
    def old():
        preds = img.new_zeros((1, K, IMG, IMG))
        count = img.new_zeros((1, 1, IMG, IMG))
        for y1, x1 in wins:
            logit = head.predict(feats, (CROP, CROP))
            preds += F.pad(logit, (x1, IMG - x1 - CROP, y1, IMG - y1 - CROP))
            count[:, :, y1:y1 + CROP, x1:x1 + CROP] += 1
        pred = (preds / count).argmax(dim=1)
        return mtp_amd.IoUMetric.total_area_to_metrics(*_areas_torch(pred[0], lab[0].to(pred)), ["mIoU"])

    # the evaluation passes alone, on the per-window logits both paths start from
    with torch.no_grad():
        rows, (_, h, w) = model.encode_decode(img[:, :, :CROP, :CROP])
        up = head.predict(feats, (CROP, CROP))
    cy = window_counts(IMG, CROP, STRIDE).to(dev)

    def eval_new():
        acc = torch.zeros(1, IMG, IMG, rows.shape[1], device=dev)
        for y1, x1 in wins:
            ops.seg_window_accumulate(rows, K, 1, h, w, acc, y1, x1, CROP, CROP)
        areas = torch.zeros(3, K, device=dev, dtype=torch.int64)
        ops.seg_argmax_areas(acc, K, cy, cy, pred=torch.empty(1, IMG, IMG, device=dev, dtype=torch.uint8), labels=lab, areas=areas)
        return areas.cpu()

    def eval_old():
        preds = img.new_zeros((1, K, IMG, IMG))
        count = img.new_zeros((1, 1, IMG, IMG))
        for y1, x1 in wins:
            preds += F.pad(up, (x1, IMG - x1 - CROP, y1, IMG - y1 - CROP))
            count[:, :, y1:y1 + CROP, x1:x1 + CROP] += 1
        return _areas_torch((preds / count).argmax(dim=1)[0], lab[0].long())

    fns = dict(new=new, old=old, eval_only_new=eval_new, eval_only_old=eval_old)
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {n: [] for n in fns}
    for _ in range(a.iters):               # alternating: both see the same machine
        for n, f in fns.items():
            ev[n].append(_events(f))
    torch.cuda.synchronize()
    ms = {n: sorted(x.elapsed_time(y) for x, y in v)[len(v) // 2] for n, v in ev.items()}
    same = float(new()["mIoU"]), float(100 * torch.as_tensor(old()["IoU"]).nanmean())
    print(json.dumps(dict(image=IMG, crop=CROP, stride=STRIDE, windows=len(wins), classes=K, head_channels=512, precision="bf16", iters=a.iters,
                          ms={n: round(v, 3) for n, v in ms.items()}, miou_new_old=[round(s, 2) for s in same],
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
