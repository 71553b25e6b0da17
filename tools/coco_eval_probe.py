"""Timing probe of the COCO-style metric (mtp_amd/evaluation/coco_metric.py on csrc/coco_eval.hip).  Device events, 2 warm-ups, the median of 10 runs.

Reports, as one JSON line:
  process_ms_per_batch   CocoMetric.process on one batch (--batch images; masks packed, box and mask IoU blocks computed)
  compute_metrics_ms     compute_metrics of metric=['bbox', 'segm'] on the synthetic set: --images images of --height x --width, --dets detections
                         and --gts gts each, --classes classes (sort -> match -> accumulate -> the one host copy -> summary)
  host_restatement_s     wall time of the numpy restatement (tests/coco_eval_ref.py: evaluateImg and accumulate for 'bbox' and 'segm') on the same
                         set, with the IoU blocks precomputed on the device and handed over
  host_syncs             synchronisations PyTorch reports under sync-debug 'warn': in process (expected 0) and in compute_metrics (expected 1)

    python tools/coco_eval_probe.py [--images 64 --dets 100 --gts 12 --classes 20 --height 256 --width 320 --batch 8]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mtp_amd import CocoMetric  # noqa: E402

WARMUP, RUNS = 2, 10


def synthetic(a, dev):
    """per image (pred, gt) dicts of device tensors: gts are random boxes with their rectangles as masks, detections are jittered gts"""
    g = torch.Generator().manual_seed(27)
    out = []
    ys, xs = torch.arange(a.height)[None, :, None], torch.arange(a.width)[None, None, :]
    for _ in range(a.images):
        wh = torch.rand(a.gts, 2, generator=g) * torch.tensor([a.width / 2.0, a.height / 2.0]) + 4
        xy = torch.rand(a.gts, 2, generator=g) * (torch.tensor([float(a.width), float(a.height)]) - wh)
        gb = torch.cat([xy, xy + wh], 1)
        pick = torch.randint(0, a.gts, (a.dets,), generator=g)
        db = gb[pick] + torch.randn(a.dets, 4, generator=g) * 3
        db[:, 2:] = torch.maximum(db[:, 2:], db[:, :2] + 1)
        gl = torch.randint(0, a.classes, (a.gts,), generator=g)
        rect = lambda b: (xs >= b[:, 0, None, None]) & (xs < b[:, 2, None, None]) & (ys >= b[:, 1, None, None]) & (ys < b[:, 3, None, None])      # noqa: E731
        out.append((dict(bboxes=db.to(dev), scores=torch.rand(a.dets, generator=g).to(dev), labels=gl[pick].to(dev), masks=rect(db).to(dev)),
                    dict(bboxes=gb.to(dev), labels=gl.to(dev), ignore_flag=(torch.rand(a.gts, generator=g) < 0.1).to(torch.uint8).to(dev), masks=rect(gb).to(dev))))
    return out


def timed(fn):
    """median of RUNS device-event times in ms after WARMUP runs"""
    ms = []
    for i in range(WARMUP + RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message) for w in seen)


def host_restatement(metric, a):
    """evaluateImg + accumulate of the restatement for 'bbox' and 'segm', the device IoU blocks handed over"""
    import coco_eval_ref as R
    images = [dict(D=im["D"], G=im["G"], scores=im["scores"].cpu().numpy().astype(np.float64), labels=im["labels"].cpu().numpy(),
                   gt_labels=im["gt_labels"].cpu().numpy(), crowd=im["gt_crowd"].cpu().numpy(), gt_area=im["gt_area"].cpu().numpy(),
                   iou={k: v.cpu().numpy().reshape(im["D"], im["G"]) for k, v in im["iou"].items()}, area={k: v.cpu().numpy() for k, v in im["area"].items()})
              for im in metric._images]
    thrs, rec, mds = np.array(metric.iou_thrs), R.Params().recThrs, metric.proposal_nums
    t0 = time.perf_counter()
    for kind in ("bbox", "segm"):
        for k in range(a.classes):
            for lo, hi in R.AREA_RNG:
                dtm, dtig, sc, rank, npig = [], [], [], [], 0
                for im in images:
                    d, g = np.nonzero(im["labels"] == k)[0], np.nonzero(im["gt_labels"] == k)[0]
                    if not len(d) and not len(g):
                        continue
                    d = d[np.argsort(-im["scores"][d], kind="mergesort")][:mds[-1]]
                    ig = (im["crowd"][g] != 0) | (im["gt_area"][g] < lo) | (im["gt_area"][g] > hi)
                    o = np.argsort(ig, kind="mergesort")
                    g, ig = g[o], ig[o].astype(np.int64)
                    npig += int((ig == 0).sum())
                    m = R.match_sequential(im["iou"][kind][np.ix_(d, g)], thrs, ig, im["crowd"][g]) if len(d) and len(g) else -np.ones((len(thrs), len(d)), np.int64)
                    out = (im["area"][kind][d] < lo) | (im["area"][kind][d] > hi)
                    dtm.append(m >= 0), dtig.append(np.where(m >= 0, ig[np.maximum(m, 0)] != 0 if len(g) else False, out[None, :]))
                    sc.append(im["scores"][d]), rank.append(np.arange(len(d)))
                if not dtm or npig == 0:
                    continue
                dtm, dtig, sc, rank = np.concatenate(dtm, 1), np.concatenate(dtig, 1), np.concatenate(sc), np.concatenate(rank)
                for md in mds:
                    R.accumulate_segment(dtm[:, rank < md], dtig[:, rank < md], sc[rank < md], npig, rec)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("images", 64), ("dets", 100), ("gts", 12), ("classes", 20), ("height", 256), ("width", 320), ("batch", 8)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    data = synthetic(a, dev)
    names = ["c%d" % k for k in range(a.classes)]
    new = lambda: CocoMetric(metric=["bbox", "segm"], classes=names)      # noqa: E731
    batch = data[:a.batch]

    def one_batch(m=None):
        m = m or new()
        m.process([p for p, _ in batch], [g for _, g in batch])
    process_ms = timed(one_batch)
    metric = new()
    sync_process = count_syncs(lambda: [metric.process([p for p, _ in data[i:i + a.batch]], [g for _, g in data[i:i + a.batch]])
                                        for i in range(0, a.images, a.batch)])
    sync_compute = count_syncs(metric.compute_metrics)
    compute_ms = timed(metric.compute_metrics)
    print(json.dumps(dict(probe="coco_eval", set=dict(images=a.images, dets_per_image=a.dets, gts_per_image=a.gts, classes=a.classes, height=a.height,
                                                      width=a.width, batch=a.batch, metrics=["bbox", "segm"], thresholds=len(metric.iou_thrs)),
                          warmup=WARMUP, runs=RUNS, process_ms_per_batch=round(process_ms, 3), compute_metrics_ms=round(compute_ms, 3),
                          host_restatement_s=round(host_restatement(metric, a), 3), host_syncs=dict(process=sync_process, compute_metrics=sync_compute))))


if __name__ == "__main__":
    main()
