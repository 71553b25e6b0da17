"""The box half of Mask R-CNN on one GPU at the workload's shape (mask_rcnn.py at bench.py's ViT-L configuration): batch 64 of 224 x 224 images, maps
of 256 channels at strides 4 / 8 / 16 / 32 / 64, A = 3 anchors per cell, 256 RPN samples and 512 RoI samples per image, nms_pre 2000, 15 classes, 8
ground truths per image.  Device-event pairs around each entry point of csrc/hbox_head.hip and around MTP_IS_RPNHead.loss_and_grads and
MTP_IS_BBoxRoIHead.loss_and_grads ('bf16' and 'fp32'), after warm-ups: median, min and max.  For the kernels the bytes the algorithm has to move
(computed from the shapes: what every launch must read once and write once) over the median give the achieved bytes/s and its share of the 8 TB/s
HBM peak.  Not a test; no ratio is asked of it.
Usage: python tools/hbox_half_probe.py [--batch 64 --iters 10 --warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mtp_amd import MODELS, ops  # noqa: E402

IMG, STRIDES, C, A, K, GTS, PEAK = 224, (4, 8, 16, 32, 64), 256, 3, 15, 8, 8e12
RPN_NUM, ROI_NUM, NMS_PRE, PROPS = 256, 512, 2000, 1000
RPN_MEANS, RPN_STDS, ROI_MEANS, ROI_STDS = (0.0,) * 4, (1.0,) * 4, (0.0,) * 4, (0.1, 0.1, 0.2, 0.2)


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


def boxes_of(rng, n, lo=8, hi=200):
    size = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    ctr = rng.uniform(0, IMG, (n, 2))
    return np.concatenate([ctr - size / 2, ctr + size / 2], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    B = a.batch
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    dev = "cuda"
    t = lambda x: torch.as_tensor(x, device=dev)      # noqa: E731
    sizes = [(-(-IMG // s), -(-IMG // s)) for s in STRIDES]
    anchors = sum(h * w * A for h, w in sizes)
    res = dict(shape=dict(batch=B, image=IMG, strides=STRIDES, channels=C, anchors_per_cell=A, anchors_per_image=anchors, rpn_samples=RPN_NUM,
                          roi_samples=ROI_NUM, nms_pre=NMS_PRE, classes=K, gts_per_image=GTS), iters=a.iters, warmup=a.warmup)
    shapes = t(np.array([[IMG, IMG]] * B, np.float32))

    # ---- the coder on plain arrays: one box per RoI sample of the batch
    n = B * ROI_NUM
    p, g, ids = t(boxes_of(rng, n)), t(boxes_of(rng, n)), t(rng.integers(0, B, n).astype(np.int64))
    d, out = torch.randn(n, 4, device=dev) * 0.5, torch.empty(n, 4, device=dev)
    res["hbox_delta_encode"] = with_rate(timed(lambda: ops.hbox_delta_encode(p, g, ROI_MEANS, ROI_STDS, out=out), a.iters, a.warmup), n * 48)
    res["hbox_delta_decode"] = with_rate(timed(lambda: ops.hbox_delta_decode(p, d, ROI_MEANS, ROI_STDS, shapes, ids, out=out), a.iters, a.warmup), n * 56)

    # ---- the RPN kernels on maps in the engine's row layout (cls in columns 0 .. A, reg in A .. 5 A of one buffer)
    ld = ops.pad8(5 * A)
    rows = sum(B * h * w for h, w in sizes)
    buf, dbuf = torch.randn(rows, ld, device=dev), torch.zeros(rows, ld, device=dev)
    row0 = np.cumsum([0] + [B * h * w for h, w in sizes])
    cls = [ops.rpn_map_rows(buf, h, w, 0, int(r)) for (h, w), r in zip(sizes, row0)]
    reg = [ops.rpn_map_rows(buf, h, w, A, int(r)) for (h, w), r in zip(sizes, row0)]
    dcls, dreg = [(dbuf,) + m[1:] for m in cls], [(dbuf,) + m[1:] for m in reg]
    priors = torch.cat([torch.as_tensor(np.stack([np.tile(np.arange(w) * s, h), np.repeat(np.arange(h) * s, w)] * 2, 1)[:, None, :] +
                                        np.array([[-4 * s, -4 * s, 4 * s, 4 * s]] * A)[None], dtype=torch.float32).reshape(-1, 4) for (h, w), s in zip(sizes, STRIDES)]).to(dev)
    gts = t(boxes_of(rng, B * GTS, 16, 160))
    samples = t(np.stack([rng.permutation(anchors)[:RPN_NUM] for _ in range(B)]).astype(np.int64))
    sample_gt = t((np.arange(B)[:, None] * GTS + rng.integers(0, GTS, (B, RPN_NUM))).astype(np.int64))
    n_pos, n_neg = torch.full((B,), RPN_NUM // 2, device=dev, dtype=torch.int64), torch.full((B,), RPN_NUM // 2, device=dev, dtype=torch.int64)
    lc, lb = torch.empty(len(sizes), device=dev), torch.empty(len(sizes), device=dev)
    # per sample: the index, the gt row, the prior, (on positives) the gt and four deltas, the logit; a gradient store for every value read from a map
    rpn_bytes = B * RPN_NUM * (16 + 16 + 2 * 4) + B * (RPN_NUM // 2) * (16 + 2 * 16)
    res["hrpn_loss"] = with_rate(timed(lambda: ops.hrpn_loss(cls, reg, sizes, A, priors, gts, samples, sample_gt, n_pos, n_neg, RPN_MEANS, RPN_STDS, dcls=dcls, dreg=dreg,
                                                             loss_cls=lc, loss_bbox=lb), a.iters, a.warmup), rpn_bytes)
    res["hrpn_loss"]["loss_rpn_cls"] = float(lc.sum())
    counts = [min(NMS_PRE, h * w * A) for h, w in sizes]
    T = sum(counts)
    keep = t(np.stack([np.concatenate([rng.permutation(h * w * A)[:k] for (h, w), k in zip(sizes, counts)]) for _ in range(B)]).astype(np.int64))
    pout = (torch.empty(B, T, device=dev), torch.empty(B, T, 4, device=dev), torch.empty(B, T, device=dev, dtype=torch.int64), torch.empty(B, T, device=dev, dtype=torch.uint8))
    # per kept anchor: the index, the logit, four deltas, the prior; score, box, level id, flag out
    res["hrpn_proposals"] = with_rate(timed(lambda: ops.hrpn_proposals(cls, reg, sizes, A, priors, keep, counts, RPN_MEANS, RPN_STDS, shapes, 0.0, out=pout), a.iters, a.warmup),
                                      B * T * (8 + 4 + 16 + 16 + 4 + 16 + 8 + 1))
    res["kept_per_image"] = T
    del buf, dbuf

    # ---- the RoI kernels on rows as the engine lays them out: K + 1 logits, then 4 K deltas from a 16-byte boundary
    R = B * ROI_NUM
    c0 = -(-(K + 1) // 4) * 4
    ldo = ops.pad8(c0 + 4 * K)
    o, do = torch.randn(R, ldo, device=dev), torch.zeros(R, ldo, device=dev)
    rois = t(np.concatenate([np.repeat(np.arange(B, dtype=np.float32), ROI_NUM)[:, None], boxes_of(rng, R)], 1))
    rgt = t((np.arange(B)[:, None] * GTS + rng.integers(0, GTS, (B, ROI_NUM))).astype(np.int64))
    labels = t(rng.integers(0, K, B * GTS).astype(np.int64))
    rp, rn = torch.full((B,), ROI_NUM // 4, device=dev, dtype=torch.int64), torch.full((B,), ROI_NUM - ROI_NUM // 4, device=dev, dtype=torch.int64)
    boxes4 = rois[:, 1:].contiguous()
    losses = torch.empty(3, device=dev)
    # per row: K + 1 logits in, K + 1 and 4 K gradients out, the RoI; on positives the gt and the label's four deltas
    roi_bytes = R * ((K + 1) * 4 * 2 + 4 * K * 4 + 16 + 8) + B * (ROI_NUM // 4) * (16 + 16 + 8)
    for mode in ("reference", "encoded"):
        res["hroi_loss_" + mode] = with_rate(timed(lambda: ops.hroi_loss(o[:, :K + 1], o[:, c0:c0 + 4 * K], K, boxes4, gts, labels, rgt, rp, rn, ROI_MEANS, ROI_STDS, mode,
                                                                         dcls=do[:, :K + 1], dreg=do[:, c0:c0 + 4 * K], losses=losses), a.iters, a.warmup), roi_bytes)
        res["hroi_loss_" + mode]["losses"] = losses.tolist()
    Rt = B * PROPS
    ot = torch.randn(Rt, ldo, device=dev)
    trois = t(np.concatenate([np.repeat(np.arange(B, dtype=np.float32), PROPS)[:, None], boxes_of(rng, Rt)], 1))
    po = (torch.empty(Rt, K, device=dev), torch.empty(Rt, K, 4, device=dev), torch.empty(Rt, K, device=dev, dtype=torch.uint8))
    # per RoI: K + 1 logits and 4 K deltas in, the RoI; K scores, K boxes and K flags out
    res["hroi_predict"] = with_rate(timed(lambda: ops.hroi_predict(ot[:, :K + 1], ot[:, c0:c0 + 4 * K], K, trois, ROI_MEANS, ROI_STDS, shapes, None, 0.05, out=po),
                                          a.iters, a.warmup), Rt * ((K + 1) * 4 + 4 * K * 4 + 20 + K * 4 + K * 16 + K))
    res["hroi_predict"]["rois"] = Rt
    del o, do, ot

    # ---- the heads: one training pass each, sampling included
    feats = [torch.randn(B, C, h, w, device=dev) for h, w in sizes]
    metas = [dict(img_shape=(IMG, IMG), pad_shape=(IMG, IMG), scale_factor=(1.0, 1.0))] * B
    gt_list = [NS(bboxes=gts[b * GTS:(b + 1) * GTS].clamp(0, IMG).contiguous(), labels=labels[b * GTS:(b + 1) * GTS].contiguous()) for b in range(B)]
    props = [NS(bboxes=t(boxes_of(rng, PROPS)).clamp(0, IMG).contiguous()) for _ in range(B)]
    gen = torch.Generator(device=dev).manual_seed(0)
    for precision in ("bf16", "fp32"):
        rpn = MODELS.build(dict(
            type="MTP_IS_RPNHead", in_channels=C, feat_channels=C, anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=list(STRIDES)),
            bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=list(RPN_MEANS), target_stds=list(RPN_STDS)), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
            train_cfg=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1),
                           sampler=dict(type="RandomSampler", num=RPN_NUM, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False), allowed_border=-1, pos_weight=-1),
            test_cfg=dict(nms_pre=NMS_PRE, max_per_img=PROPS, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0), precision=precision)).to(dev)
        res["rpn_loss_and_grads_" + precision] = timed(lambda: rpn.loss_and_grads(feats, gt_list, metas, generator=gen), a.iters, a.warmup)
        del rpn
        roi = MODELS.build(dict(
            type="MTP_IS_BBoxRoIHead",
            bbox_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0), out_channels=C,
                                    featmap_strides=list(STRIDES[:4])),
            bbox_head=dict(type="MTP_IS_Shared2FCBBoxHead", in_channels=C, fc_out_channels=1024, roi_feat_size=7, num_classes=K,
                           bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=list(ROI_MEANS), target_stds=list(ROI_STDS)), precision=precision),
            train_cfg=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=True, ignore_iof_thr=-1),
                           sampler=dict(type="RandomSampler", num=ROI_NUM, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1))).to(dev)
        res["roi_loss_and_grads_" + precision] = timed(lambda: roi.loss_and_grads(feats, props, gt_list, generator=gen), a.iters, a.warmup)
        res["roi_loss_and_grads_" + precision]["loss_cls"] = float(roi.loss(feats, props, gt_list, generator=gen)["loss_cls"])
        del roi
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
