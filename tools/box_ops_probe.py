"""The box operators at the detection workload's shapes on one GPU, each against the torch composition of the same semantics: device-event pairs
after a warm-up, the two alternating in one process; medians and the spread.  Not a test.
  * NMS over 5 x 2000 boxes with level ids at 0.7 (the RPN's batched_nms): sort + mask + scan + the count's host sync, and the mask and scan launches
    on their own.  The composition: broadcast IoU on the device with the ids folded in, the matrix copied to the host, the greedy loop there (torch has
    no device statement of the sequential rule).
  * MaxIoU assignment, K = 100 gts, N = 262144 priors (1024 x 1024, FPN strides 4 to 64, three anchors), box / box and rotated / rotated, the RPN's
    configuration (0.7 / 0.3 / 0.3, low-quality matching on): the fused two-phase kernels, and phase one alone (match_low_quality off).  The composition:
    the K x N matrix (broadcast IoU in torch; for rotated boxes, which torch cannot state, this library's pairwise kernel) + assign_wrt_overlaps in torch.
Usage: python tools/box_ops_probe.py [--iters 30 --warmup 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mtp_amd import MaxIoUAssigner, batched_nms, ops  # noqa: E402


def timed(fns, iters, warmup):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    names = list(fns)
    for i in range(iters):
        for name in (names if i % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[name]()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: dict(median=statistics.median(t), min=min(t), max=max(t)) for k, t in times.items()}


def torch_iou(a, b):
    lt, rb = torch.max(a[:, None, :2], b[None, :, :2]), torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    aa, ab = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (aa[:, None] + ab[None] - inter).clamp(min=1e-6)


def boxes(n, rng, size, lo, hi, rotated):
    c, wh = rng.uniform(hi / 2, size - hi / 2, (n, 2)), rng.uniform(lo, hi, (n, 2))
    b = np.concatenate([c, wh, rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1) if rotated else np.concatenate([c - wh / 2, c + wh / 2], 1)
    return torch.from_numpy(b.astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    rng = np.random.default_rng(0)
    res = {}

    # ---- NMS: 5 levels x 2000 proposals, clustered around 100 objects so that suppression chains form as they do behind an RPN
    n = 10000
    centres = boxes(100, rng, 1024, 32, 256, False)
    b = centres[torch.from_numpy(rng.integers(0, 100, n)).cuda()] + torch.from_numpy(rng.normal(0, 6, (n, 4)).astype(np.float32)).cuda()
    b[:, 2:] = torch.maximum(b[:, 2:], b[:, :2] + 1)
    scores = torch.from_numpy(rng.permutation(n).astype(np.float32) / n).cuda()
    ids = torch.arange(n, device="cuda") // 2000
    cfg = dict(type="nms", iou_threshold=0.7)
    order = torch.sort(scores, descending=True, stable=True)[1]
    bs, gs = b[order].contiguous(), ids[order].contiguous()
    mask = torch.empty(n * ((n + 63) // 64), device="cuda", dtype=torch.int64)
    keep, count = torch.empty(n, device="cuda", dtype=torch.int64), torch.empty(1, device="cuda", dtype=torch.int64)
    lib, s = ops.lib(), ops._s

    def composed_nms():
        m = (torch_iou(bs, bs) > 0.7) & (gs[:, None] == gs[None])
        m = m.cpu().numpy()
        dead, out = np.zeros(n, bool), []
        for i in range(n):
            if not dead[i]:
                out.append(i)
                dead |= m[i]
        return order[torch.as_tensor(out, device="cuda")]
    fused_keep = batched_nms(b, scores, ids, cfg)[1]
    same = bool(torch.equal(fused_keep, composed_nms()))
    res["nms_5x2000_thr0.7"] = dict(kept=int(fused_keep.numel()), same_list_as_the_composition=same, **timed({
        "fused_batched_nms_us": lambda: batched_nms(b, scores, ids, cfg),
        "mask_launch_us": lambda: lib.mtp_nms_mask(bs.data_ptr(), gs.data_ptr(), n, 0, 0.7, mask.data_ptr(), mask.numel() * 8, s()),
        "scan_launch_us": lambda: lib.mtp_nms_scan(mask.data_ptr(), n, n, keep.data_ptr(), count.data_ptr(), s()),
    }, a.iters, a.warmup))
    res["nms_5x2000_thr0.7"].update(timed({"torch_iou_matrix_plus_host_loop_us": composed_nms}, 3, 1))

    # ---- assignment: K = 100, N = 262144
    K, N = 100, 262144
    for kind, rot in (("box", False), ("rotated", True)):
        gts, priors = boxes(K, rng, 1024, 16, 256, rot), boxes(N, rng, 1024, 16, 256, rot)
        priors[:K] = gts + 2.0 * (0.0 if rot else 1.0)      # some positives
        labels = torch.from_numpy(rng.integers(0, 15, K)).cuda()
        calc = "RBboxOverlaps2D" if rot else "BboxOverlaps2D"
        asg = MaxIoUAssigner(0.7, 0.3, 0.3, iou_calculator=dict(type=calc))

        def matrix():
            return ops.box_iou(gts, priors, rotated=True) if rot else torch_iou(gts, priors)
        want = asg.assign_wrt_overlaps(matrix(), labels)
        got = ops.max_iou_assign(gts, priors, labels, kind, 0.7, 0.3, 0.3, True, True)
        agree = float((got[0] == want.gt_inds).float().mean())
        res["assign_%s_K100_N262144" % kind] = dict(gt_inds_agreement_with_the_f32_matrix=agree, positives=int((got[0] > 0).sum()), **timed({
            "fused_two_phases_us": lambda: ops.max_iou_assign(gts, priors, labels, kind, 0.7, 0.3, 0.3, True, True),
            "fused_phase_one_only_us": lambda: ops.max_iou_assign(gts, priors, labels, kind, 0.7, 0.3, 0.3, False, True),
            "matrix_plus_assign_wrt_overlaps_us": lambda: asg.assign_wrt_overlaps(matrix(), labels),
            "matrix_only_us": matrix,
        }, a.iters, a.warmup))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
