"""The oriented RoI head at the detection workload's shape on one GPU -- 1024 x 1024, batch 2, 40 gts and 2000 proposals per image, four maps of
256 channels at strides 4 to 32, num=512, fc_out_channels=1024, 15 classes -- each path against a torch composition of the same steps on the same
GPU: device-event pairs after a warm-up, the two alternating in one process; medians and the spread.  Not a test.
  * RoIAlignRotated forward and backward over the 1024 sampled RoIs (one launch; entries, a stable sort and one gather launch) against: the level
    loop with nonzero() of the reference's extractor, the sample grid and the bilinear rules in torch, four gathers, and autograd's backward
    (index_put with accumulate, i.e. float atomics).
  * the whole StandardRoIHead.loss_and_grads against: the K x N rotated overlaps (mtp_amd.box_iou_rotated: torch has none), assign_wrt_overlaps,
    nonzero / randperm sampling with the gts prepended, that RoIAlignRotated, nn.Linear layers, cross_entropy, the delta encode, smooth_l1_loss and
    autograd's backward.
Usage: python tools/roi_probe.py [--iters 20 --warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from box_ops_probe import timed  # noqa: E402
from mtp_amd import MODELS, box_iou_rotated  # noqa: E402

SIZE, BATCH, GTS, PROPS, NUM, C, FC, K, P, S = 1024, 2, 40, 2000, 512, 256, 1024, 15, 7, 2
STRIDES, FINEST = (4, 8, 16, 32), 56
MEANS, STDS = (0.0,) * 5, (0.1, 0.1, 0.2, 0.2, 0.1)


def norm_angle(a):
    return torch.remainder(a + np.pi / 2, np.pi) - np.pi / 2


def encode_t(p, g):
    cs, sn = torch.cos(p[:, 4]), torch.sin(p[:, 4])
    ex, ey = g[:, 0] - p[:, 0], g[:, 1] - p[:, 1]
    d1, d2 = norm_angle(g[:, 4] - p[:, 4]), norm_angle(g[:, 4] - p[:, 4] + np.pi / 2)
    first = d1.abs() < d2.abs()
    d = torch.stack([(cs * ex + sn * ey) / p[:, 2], (-sn * ex + cs * ey) / p[:, 3], torch.log(torch.where(first, g[:, 2], g[:, 3]) / p[:, 2]),
                     torch.log(torch.where(first, g[:, 3], g[:, 2]) / p[:, 3]), torch.where(first, d1, d2)], 1)
    return (d - d.new_tensor(MEANS)) / d.new_tensor(STDS)


def align_level_t(feat, rois, scale):
    """feat (N, C, H, W), rois (n, 6) -> (n, C, P, P): mmcv's roi_align_rotated (aligned, clockwise) in torch"""
    H, W = feat.shape[2:]
    b = rois[:, 0].long()
    cx, cy, rw, rh, th = rois[:, 1] * scale - 0.5, rois[:, 2] * scale - 0.5, rois[:, 3] * scale, rois[:, 4] * scale, -rois[:, 5]
    cs, sn = torch.cos(th)[:, None, None], torch.sin(th)[:, None, None]
    bins, sub = torch.arange(P * P, device=feat.device), torch.arange(S * S, device=feat.device)
    ph, pw, iy, ix = (bins // P).float()[None, :, None], (bins % P).float()[None, :, None], (sub // S).float()[None, None, :], (sub % S).float()[None, None, :]
    bh, bw = (rh / P)[:, None, None], (rw / P)[:, None, None]
    yy = -rh[:, None, None] / 2 + ph * bh + (iy + 0.5) * bh / S
    xx = -rw[:, None, None] / 2 + pw * bw + (ix + 0.5) * bw / S
    y, x = yy * cs - xx * sn + cy[:, None, None], yy * sn + xx * cs + cx[:, None, None]
    inside = (y >= -1) & (y <= H) & (x >= -1) & (x <= W)
    y, x = y.clamp(min=0), x.clamp(min=0)
    yl, xl = y.long().clamp(max=H - 1), x.long().clamp(max=W - 1)
    yh, xh = (yl + 1).clamp(max=H - 1), (xl + 1).clamp(max=W - 1)
    y, x = torch.where(yl >= H - 1, yl.float(), y), torch.where(xl >= W - 1, xl.float(), x)
    ly, lx = y - yl, x - xl
    hy, hx = 1 - ly, 1 - lx
    f = feat.permute(0, 2, 3, 1)      # (N, H, W, C)
    bb = b[:, None, None].expand_as(yl)
    val = ((hy * hx)[..., None] * f[bb, yl, xl] + (hy * lx)[..., None] * f[bb, yl, xh] + (ly * hx)[..., None] * f[bb, yh, xl] + (ly * lx)[..., None] * f[bb, yh, xh])
    out = (val * inside[..., None]).sum(2) / (S * S)      # (n, P P, C)
    return out.permute(0, 2, 1).reshape(-1, feat.shape[1], P, P)


def align_t(feats, rois):
    lv = torch.floor(torch.log2(torch.sqrt(rois[:, 3] * rois[:, 4]) / FINEST + 1e-6)).clamp(0, len(feats) - 1).long()
    out = feats[0].new_zeros(rois.shape[0], feats[0].shape[1], P, P)
    for l, f in enumerate(feats):
        idx = torch.nonzero(lv == l).squeeze(1)
        if idx.numel():
            out[idx] = align_level_t(f, rois[idx], 1.0 / STRIDES[l])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    rng = np.random.default_rng(0)
    head = MODELS.build(dict(
        type="MTP_RD_StandardRoIHead",
        bbox_roi_extractor=dict(type="RotatedSingleRoIExtractor", roi_layer=dict(type="RoIAlignRotated", out_size=P, sample_num=S, clockwise=True), out_channels=C,
                                featmap_strides=list(STRIDES)),
        bbox_head=dict(type="MTP_RD_Shared2FCBBoxHead", in_channels=C, fc_out_channels=FC, roi_feat_size=P, num_classes=K,
                       bbox_coder=dict(type="mmrotate.DeltaXYWHTRBBoxCoder", angle_version="le90", norm_factor=None, edge_swap=True, proj_xy=True,
                                       target_means=MEANS, target_stds=STDS)),
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1,
                                     iou_calculator=dict(type="mmrotate.RBboxOverlaps2D")),
                       sampler=dict(type="RandomSampler", num=NUM, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1),
        test_cfg=dict(score_thr=0.05, nms=dict(type="nms_rotated", iou_threshold=0.1), max_per_img=2000))).cuda()
    feats = [torch.from_numpy(rng.normal(0, 1, (BATCH, C, SIZE // s, SIZE // s)).astype(np.float32)).cuda() for s in STRIDES]
    gts, props = [], []
    for _ in range(BATCH):
        g = np.concatenate([rng.uniform(100, 924, (GTS, 2)), rng.uniform(16, 300, (GTS, 2)), rng.uniform(-1.5, 1.5, (GTS, 1))], 1)
        near = g[rng.integers(0, GTS, PROPS // 2)] * rng.uniform(0.9, 1.1, (PROPS // 2, 5))
        far = np.concatenate([rng.uniform(0, SIZE, (PROPS - PROPS // 2, 2)), rng.uniform(8, 500, (PROPS - PROPS // 2, 2)), rng.uniform(-1.5, 1.5, (PROPS - PROPS // 2, 1))], 1)
        gts.append(torch.from_numpy(g.astype(np.float32)).cuda())
        props.append(torch.from_numpy(np.concatenate([near, far]).astype(np.float32)).cuda())
    labels = [torch.from_numpy(rng.integers(0, K, GTS)).cuda() for _ in range(BATCH)]
    inst = [NS(rboxes=g, rlabels=l) for g, l in zip(gts, labels)]
    rpn = [NS(bboxes=p) for p in props]
    ex, bh = head.bbox_roi_extractor, head.bbox_head
    s = head.gen_sampling_results(rpn, inst, generator=torch.Generator(device="cuda").manual_seed(0))
    rois, valid = s["rois"], (s["n_pos"] + s["n_neg"]).contiguous()
    rows, maps, sizes, images = head._levels(feats)
    dout = torch.randn(rois.shape[0], P * P, C, device="cuda")
    drows = [torch.zeros_like(r) for r in rows]
    dmaps = [(d,) + m[1:] for d, m in zip(drows, maps)]

    def fused_fwd():
        return ex.extract(maps, sizes, images, rois, valid=valid)

    def fused_bwd():
        for d in drows:
            d.zero_()
        return ex.extract_bwd(dout, dmaps, sizes, images, rois, valid=valid)

    leaf = [f.clone().requires_grad_() for f in feats]
    dout_t = dout.permute(0, 2, 1).reshape(-1, C, P, P).contiguous()

    def torch_fwd():
        with torch.no_grad():
            return align_t(feats, rois)

    def torch_fwd_bwd():
        for f in leaf:
            f.grad = None
        align_t(leaf, rois).backward(dout_t)
        return [f.grad for f in leaf]

    def fused_step():
        return head.loss_and_grads(feats, rpn, inst)

    lin = [torch.nn.Linear(C * P * P, FC).cuda(), torch.nn.Linear(FC, FC).cuda(), torch.nn.Linear(FC, K + 1).cuda(), torch.nn.Linear(FC, 5).cuda()]

    def composed_step():
        for f in leaf:
            f.grad = None
        for m in lin:
            m.zero_grad(set_to_none=True)
        all_rois, all_lab, all_tgt, all_w = [], [], [], []
        for b, (g, lab, p) in enumerate(zip(gts, labels, props)):
            res = head.bbox_assigner.assign_wrt_overlaps(box_iou_rotated(g, p), lab)
            boxes = torch.cat([g, p])
            gt_inds = torch.cat([torch.arange(1, GTS + 1, device="cuda"), res.gt_inds])
            pos = torch.nonzero(gt_inds > 0).squeeze(1)
            if pos.numel() > NUM // 4:
                pos = pos[torch.randperm(pos.numel())[:NUM // 4].to(pos.device)]
            neg = torch.nonzero(gt_inds == 0).squeeze(1)
            if neg.numel() > NUM - pos.numel():
                neg = neg[torch.randperm(neg.numel())[:NUM - pos.numel()].to(neg.device)]
            idx = torch.cat([pos, neg])
            r = boxes[idx]
            all_rois.append(torch.cat([r.new_full((r.shape[0], 1), float(b)), r], 1))
            all_lab.append(torch.cat([lab[gt_inds[pos] - 1], lab.new_full((neg.numel(),), K)]))
            tgt, w = r.new_zeros(r.shape[0], 5), r.new_zeros(r.shape[0], 5)
            tgt[:pos.numel()] = encode_t(r[:pos.numel()], g[gt_inds[pos] - 1])
            w[:pos.numel()] = 1.0
            all_tgt.append(tgt)
            all_w.append(w)
        rr, lab, tgt, w = torch.cat(all_rois), torch.cat(all_lab), torch.cat(all_tgt), torch.cat(all_w)
        x = align_t(leaf, rr).flatten(1)
        y = F.relu(lin[1](F.relu(lin[0](x))))
        loss = F.cross_entropy(lin[2](y), lab) + (F.smooth_l1_loss(lin[3](y), tgt, beta=1.0, reduction="none") * w).sum() / rr.shape[0]
        loss.backward()
        return loss

    res = dict(shape=dict(size=SIZE, batch=BATCH, gts=GTS, proposals=PROPS, num=NUM, channels=C, fc_out_channels=FC, classes=K, rois=int(rois.shape[0]),
                          rois_in_use=int(valid.sum())))
    fa, ta = fused_fwd(), torch_fwd()
    res["roi_align_fwd"] = dict(max_difference=float((fa.permute(0, 2, 1).reshape(ta.shape) - ta).abs().max()),
                                **timed({"fused_us": fused_fwd, "torch_composition_us": torch_fwd}, a.iters, a.warmup))
    res["roi_align_fwd_bwd"] = timed({"fused_bwd_only_us": fused_bwd, "torch_composition_fwd_and_bwd_us": torch_fwd_bwd}, a.iters, a.warmup)
    fl = fused_step()
    res["loss_and_grads"] = dict(fused_total=float(fl[0]["loss_cls"] + fl[0]["loss_bbox"]), composed_total=float(composed_step().detach()),      # other weights, other draws
                                 **timed({"fused_us": fused_step, "torch_composition_us": composed_step}, a.iters, a.warmup))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
