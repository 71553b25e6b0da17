"""The oriented RPN at the detection workload's shape on one GPU -- 1024 x 1024, batch 2, 40 gts per image, strides 4 to 64 with three anchors
(261888 anchors), num=256, nms_pre = max_per_img = 2000 -- each path against the torch composition of the same steps, indexed as the reference
indexes (rotated_detection/anchor_head.py, random_sampler.py, rpn_head.py): device-event pairs after a warm-up, the two alternating in one process;
medians and the spread.  Not a test.
  * targets + loss, forward and backward on given maps: OrientedRPNHead.loss_by_feat(return_grads=True) (fused assigner, the sampler without a
    synchronisation, the two launches of mtp_rpn_loss) against: boolean-mask inside anchors, the K x N matrix, assign_wrt_overlaps, nonzero /
    randperm / unique, encode, unmap, images_to_levels, per-level BCE and SmoothL1 and autograd's backward.
  * proposals: OrientedRPNHead.predict_by_feat (per-level sort, one decode launch, NMS image by image) against: per level sigmoid, sort, gather,
    decode in torch, boolean-mask size filter, then the SAME NMS kernels (torch has no device statement of the sequential rule).
Usage: python tools/rpn_probe.py [--iters 20 --warmup 3] [--out FILE]"""
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
from box_ops_probe import timed, torch_iou  # noqa: E402
from mtp_amd import MODELS, batched_nms  # noqa: E402
from mtp_amd.task_modules.iou_calculators import rbox2hbox  # noqa: E402

SIZE, BATCH, K, NUM, A = 1024, 2, 40, 256, 3
STRIDES = (4, 8, 16, 32, 64)
MEANS, STDS, BETA = (0.0,) * 6, (1.0, 1.0, 1.0, 1.0, 0.5, 0.5), 1.0 / 9.0
PROPOSAL = dict(nms_pre=2000, max_per_img=2000, nms=dict(type="nms", iou_threshold=0.8), min_bbox_size=0)
MAX_RATIO = abs(np.log(16 / 1000))


def encode_t(p, g):
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    hb = rbox2hbox(g)
    gx, gy, gw, gh = (hb[:, 0] + hb[:, 2]) * 0.5, (hb[:, 1] + hb[:, 3]) * 0.5, hb[:, 2] - hb[:, 0], hb[:, 3] - hb[:, 1]
    hw, hh, c, s = g[:, 2] * 0.5, g[:, 3] * 0.5, torch.cos(g[:, 4]), torch.sin(g[:, 4])
    ux, uy, vx, vy = hw * c, hw * s, -(hh * s), hh * c
    X = torch.stack([g[:, 0] - ux - vx, g[:, 0] + ux - vx, g[:, 0] + ux + vx, g[:, 0] - ux + vx], 1)
    Y = torch.stack([g[:, 1] - uy - vy, g[:, 1] + uy - vy, g[:, 1] + uy + vy, g[:, 1] - uy + vy], 1)
    xa, ya = X.clone(), Y.clone()
    xa[(Y - Y.min(1, keepdim=True)[0]).abs() > 0.1] = -1000
    ya[(X - X.max(1, keepdim=True)[0]).abs() > 0.1] = -1000
    ga, gb = xa.max(1)[0], ya.max(1)[0]
    d = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph), (ga - gx) / gw, (gb - gy) / gh], 1)
    return (d - d.new_tensor(MEANS)) / d.new_tensor(STDS)


def decode_t(p, raw):
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    d = raw * raw.new_tensor(STDS) + raw.new_tensor(MEANS)
    dw, dh = d[:, 2].clamp(-MAX_RATIO, MAX_RATIO), d[:, 3].clamp(-MAX_RATIO, MAX_RATIO)
    gw, gh, gx, gy = pw * dw.exp(), ph * dh.exp(), px + pw * d[:, 0], py + ph * d[:, 1]
    da, db = d[:, 4].clamp(-0.5, 0.5), d[:, 5].clamp(-0.5, 0.5)
    c0, c1 = torch.stack([da * gw, -gh * 0.5], 1), torch.stack([gw * 0.5, db * gh], 1)
    n0, n1 = c0.norm(dim=1, keepdim=True), c1.norm(dim=1, keepdim=True)
    diag = torch.maximum(n0, n1)
    v0, v1 = c0 * diag / n0, c1 * diag / n1
    e1, e2 = v1 - v0, v1 + v0
    l1, l2 = e1.norm(dim=1), e2.norm(dim=1)
    first = l1 >= l2
    e = torch.where(first[:, None], e1, e2)
    t = torch.atan2(e[:, 1], e[:, 0])
    t = torch.where(t >= np.pi / 2, t - np.pi, t)
    t = torch.where(t < -np.pi / 2, t + np.pi, t)
    return torch.stack([gx, gy, torch.where(first, l1, l2), torch.where(first, l2, l1), t], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs the MI355X"
    rng = np.random.default_rng(0)
    head = MODELS.build(dict(
        type="OrientedRPNHead", in_channels=256, feat_channels=256,
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1,
                                     iou_calculator=dict(type="mmrotate.RBbox2HBboxOverlaps2D")),
                       sampler=dict(type="RandomSampler", num=NUM, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False), allowed_border=0, pos_weight=-1),
        test_cfg=PROPOSAL)).cuda()
    sizes = [(SIZE // s, SIZE // s) for s in STRIDES]
    cls = [torch.from_numpy(rng.normal(0, 1.5, (BATCH, A, H, W)).astype(np.float32)).cuda() for H, W in sizes]
    reg = [torch.from_numpy(rng.normal(0, 0.3, (BATCH, 6 * A, H, W)).astype(np.float32)).cuda() for H, W in sizes]
    gts = [torch.from_numpy(np.concatenate([rng.uniform(100, 924, (K, 2)), rng.uniform(16, 200, (K, 2)), rng.uniform(-1.5, 1.5, (K, 1))], 1).astype(np.float32)).cuda()
           for _ in range(BATCH)]
    labels = torch.zeros(K, dtype=torch.int64, device="cuda")
    metas = [dict(img_shape=(SIZE, SIZE), pad_shape=(SIZE, SIZE)) for _ in range(BATCH)]
    inst = [NS(rboxes=g, rlabels=labels) for g in gts]
    lv = head.prior_generator.priors_and_flags(sizes, (SIZE, SIZE), (SIZE, SIZE), 0, "cuda")
    flat, flags = torch.cat([p for p, _ in lv]), torch.cat([f for _, f in lv]).bool()
    counts = [p.shape[0] for p, _ in lv]

    def fused_loss():
        return head.loss_by_feat(cls, reg, inst, metas, return_grads=True)

    def composed_loss():
        c, r = [m.clone().requires_grad_() for m in cls], [m.clone().requires_grad_() for m in reg]
        per_image, avg = [], 0
        for g in gts:
            anchors = flat[flags]
            res = head.assigner.assign_wrt_overlaps(torch_iou(rbox2hbox(g), anchors), labels)
            pos = torch.nonzero(res.gt_inds > 0).squeeze(1)
            if pos.numel() > NUM // 2:
                pos = pos[torch.randperm(pos.numel())[:NUM // 2].to(pos.device)]
            pos = pos.unique()
            neg = torch.nonzero(res.gt_inds == 0).squeeze(1)
            if neg.numel() > NUM - pos.numel():
                neg = neg[torch.randperm(neg.numel())[:NUM - pos.numel()].to(neg.device)]
            neg = neg.unique()
            n = anchors.shape[0]
            lab, lw = anchors.new_full((n,), 1, dtype=torch.long), anchors.new_zeros(n)
            bt, bw = anchors.new_zeros(n, 6), anchors.new_zeros(n, 6)
            if len(pos) > 0:
                bt[pos] = encode_t(anchors[pos], g[res.gt_inds[pos] - 1])
                bw[pos] = 1.0
                lab[pos] = 0
                lw[pos] = 1.0
            if len(neg) > 0:
                lw[neg] = 1.0
            full = []
            for t, fill in ((lab, 1), (lw, 0), (bt, 0), (bw, 0)):      # unmap
                u = t.new_full((flat.shape[0],) + tuple(t.shape[1:]), fill)
                u[flags] = t
                full.append(u)
            per_image.append(full)
            avg += pos.numel() + neg.numel()
        total, first = 0.0, 0
        for l, n in enumerate(counts):      # images_to_levels, loss_by_feat_single
            lab, lw, bt, bw = (torch.stack([img[i][first:first + n] for img in per_image]) for i in range(4))
            z = c[l].permute(0, 2, 3, 1).reshape(-1)
            total = total + F.binary_cross_entropy_with_logits(z, (lab.reshape(-1) == 0).float(), weight=lw.reshape(-1), reduction="sum") / avg
            d = r[l].permute(0, 2, 3, 1).reshape(-1, 6)
            total = total + (F.smooth_l1_loss(d, bt.reshape(-1, 6), beta=BETA, reduction="none") * bw.reshape(-1, 6)).sum() / avg
            first += n
        total.backward()
        return total, [m.grad for m in c], [m.grad for m in r]

    def fused_proposals():
        return head.predict_by_feat(cls, reg, batch_img_metas=metas)

    def composed_proposals():
        out, first_of = [], np.cumsum([0] + counts)
        for b in range(BATCH):
            boxes, scores, ids = [], [], []
            for l in range(len(sizes)):
                s = cls[l][b].permute(1, 2, 0).reshape(-1).sigmoid()
                d = reg[l][b].permute(1, 2, 0).reshape(-1, 6)
                pri = flat[first_of[l]:first_of[l + 1]]
                if 0 < PROPOSAL["nms_pre"] < s.shape[0]:
                    ranked, rank = s.sort(descending=True)
                    top = rank[:PROPOSAL["nms_pre"]]
                    s, d, pri = ranked[:PROPOSAL["nms_pre"]], d[top], pri[top]
                boxes.append(decode_t(pri, d))
                scores.append(s)
                ids.append(s.new_full((s.shape[0],), l, dtype=torch.long))
            boxes, scores, ids = torch.cat(boxes), torch.cat(scores), torch.cat(ids)
            ok = (boxes[:, 2] > PROPOSAL["min_bbox_size"]) & (boxes[:, 3] > PROPOSAL["min_bbox_size"])
            if not ok.all():
                boxes, scores, ids = boxes[ok], scores[ok], ids[ok]
            keep = batched_nms(rbox2hbox(boxes), scores, ids, PROPOSAL["nms"])[1][:PROPOSAL["max_per_img"]]
            out.append((boxes[keep], scores[keep]))
        return out

    res = dict(shape=dict(size=SIZE, batch=BATCH, gts=K, anchors=int(flat.shape[0]), inside=int(flags.sum()), num=NUM, **{k: v for k, v in PROPOSAL.items() if k != "nms"}))
    fl, cl = fused_loss(), composed_loss()
    res["targets_and_loss"] = dict(
        fused_total=float(sum(fl[0]["loss_rpn_cls"]) + sum(fl[0]["loss_rpn_bbox"])), composed_total=float(cl[0].detach()),      # different random draws
        **timed({"fused_us": fused_loss, "torch_composition_us": composed_loss}, a.iters, a.warmup))
    fp, cp = fused_proposals(), composed_proposals()
    res["proposals"] = dict(
        kept=[int(r.scores.numel()) for r in fp], composed_kept=[int(s.numel()) for _, s in cp],
        max_box_difference=[float((r.bboxes[:50] - bx[:50]).abs().max()) for r, (bx, _) in zip(fp, cp)],
        **timed({"fused_us": fused_proposals, "torch_composition_us": composed_proposals}, a.iters, a.warmup))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
