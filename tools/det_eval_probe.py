"""DOTAMetric.compute_metrics on one GPU at a DOTA-sized synthetic set: 2000 images, 15 classes, up to 2000 detections and 200 gts per image (both
counts uniform).  Device-event pairs around compute_metrics after warm-ups, the two eval modes alternating in one process: median, min and max; the
number of host synchronisations one call makes (sync-debug 'warn', counted).  Against it, once: the host loop of tests/det_eval_ref.py (tpfp_default
per class and image, the global sort, average_precision) with the IoU matrices taken from this library's kernel beforehand, so that the loop alone is
timed (wall clock).  Not a test; no ratio is asked of it.
Usage: python tools/det_eval_probe.py [--images 2000 --iters 10 --warmup 2] [--no-host-loop] [--out FILE]"""
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
import det_eval_ref as R  # noqa: E402
from mtp_amd import DOTAMetric, ops  # noqa: E402

K, MAX_DETS, MAX_GTS, CELL = 15, 2000, 200, 120.0


def scene(rng, images):
    """per image (dets (m, 5), scores (m), labels (m), gts (n, 5), gt labels (n), ignored (n) bool): gts in cells 120 px apart, 70 % of the detections
    jittered copies of gts with their label, the rest background"""
    out = []
    for _ in range(images):
        n, m = int(rng.integers(1, MAX_GTS + 1)), int(rng.integers(0, MAX_DETS + 1))
        cell = np.arange(n)
        c = np.stack([cell % 15, cell // 15], 1) * CELL + 60.0 + rng.uniform(-10, 10, (n, 2))
        gts = np.concatenate([c, rng.uniform(8, 64, (n, 2)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1)
        gl = rng.integers(0, K, n)
        src = rng.integers(0, n, m)
        dets = gts[src] + rng.uniform(-1, 1, (m, 5)) * np.concatenate([0.25 * gts[src, 2:4], 0.2 * gts[src, 2:4], np.full((m, 1), 0.15)], 1)
        dl = np.where(rng.uniform(size=m) < 0.7, gl[src], rng.integers(0, K, m))
        dets[:, 2:4] = np.maximum(dets[:, 2:4], 4.0)
        out.append((dets.astype(np.float32), rng.uniform(size=m).astype(np.float32), dl.astype(np.int64), gts.astype(np.float32), gl.astype(np.int64),
                    rng.uniform(size=n) < 0.1))
    return out


def fill(metric, data):
    for dets, scores, dl, gts, gl, ign in data:
        metric.process(dict(bboxes=dets, scores=scores, labels=dl), dict(bboxes=gts[~ign], labels=gl[~ign]), dict(bboxes=gts[ign], labels=gl[ign]))


def host_loop(host, ious, thrs):
    """det_eval_ref.compute_metrics with the per-image IoU matrices given: (seconds, metrics)"""
    det_results, annotations, lookup = [], [], {}
    for i, (dets, scores, dl, gts, gl, ign) in enumerate(host):
        d6 = np.concatenate([dets, scores[:, None]], 1).astype(np.float64)
        det_results.append([d6[dl == k] for k in range(K)])
        annotations.append(dict(bboxes=gts[~ign].astype(np.float64), labels=gl[~ign], bboxes_ignore=gts[ign].astype(np.float64), labels_ignore=gl[ign]))
        stacked = np.concatenate([np.nonzero(~ign)[0], np.nonzero(ign)[0]])
        for k in range(K):
            rows, cols = np.nonzero(dl == k)[0], stacked[gl[stacked] == k]
            if len(rows) and len(cols):      # keyed by what tpfp_default hands to iou_fn: the class's first detection and first gt
                lookup[(dets[rows[0]].tobytes(), gts[cols[0]].tobytes(), len(rows), len(cols))] = ious[i][np.ix_(rows, cols)]

    def iou_fn(d, g):
        return lookup[(d[0].tobytes(), g[0].tobytes(), len(d), len(g))]
    t0 = time.perf_counter()
    got = R.compute_metrics(det_results, annotations, thrs, iou_fn=iou_fn)
    return time.perf_counter() - t0, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    thrs = [0.5, 0.75]
    host = scene(np.random.default_rng(0), a.images)
    data = [tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in img) for img in host]
    metrics = {mode: DOTAMetric(iou_thrs=thrs, eval_mode=mode, classes=["c%d" % k for k in range(K)]) for mode in ("11points", "area")}
    for m in metrics.values():
        fill(m, data)
    tables = metrics["11points"].tables()
    res = dict(images=a.images, classes=K, detections=int(tables[0].shape[0]), gts=int(tables[4].shape[0]), iou_thrs=thrs)
    for _ in range(a.warmup):
        for m in metrics.values():
            m.compute_metrics()
    torch.cuda.synchronize()
    times = {mode: [] for mode in metrics}
    for i in range(a.iters):
        for mode in (list(metrics) if i % 2 == 0 else list(metrics)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = metrics[mode].compute_metrics()
            e1.record()
            e1.synchronize()
            times[mode].append(e0.elapsed_time(e1))
            res["metrics_" + mode] = dict(out)
    for mode, t in times.items():
        res["compute_metrics_%s_ms" % mode] = dict(median=statistics.median(t), min=min(t), max=max(t))
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        metrics["11points"].compute_metrics()
    torch.cuda.set_sync_debug_mode("default")
    res["host_syncs_per_compute_metrics"] = sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message) for w in seen)
    if not a.no_host_loop:
        ious = [ops.box_iou(d[0], d[3], rotated=True).cpu().numpy() if d[0].shape[0] else np.zeros((0, d[3].shape[0]), np.float32) for d in data]
        secs, got = host_loop(host, ious, thrs)
        res["det_eval_ref_host_loop_s"] = secs
        res["host_loop_same_metrics"] = dict(got) == res["metrics_11points"]
        res["metrics_host_loop"] = dict(got)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
