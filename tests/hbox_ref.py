"""Numpy restatement of the box half of Mask R-CNN (csrc/hbox_head.hip) for the tests of mtp_amd.dense_heads.RPNHead, mtp_amd.roi_heads.hbox_* and
mtp_amd.task_modules.DeltaXYWHBBoxCoder: the sibling of rpn_ref.py and roi_ref.py, whose steps it reuses where they already state one.  Plain helper
module: no tests, no fixtures.  Everything takes a `dtype`: float64 is the reference, float32 the same operations in the kernels' precision and
order -- its distance from float64 sets the tolerance of the GPU tests.
  * encode / decode: mmdet 3.x bbox2delta / delta2bbox (DeltaXYWHBBoxCoder), restated from the published algorithm;
  * rpn_loss: sigmoid BCE with logits and L1 over sampled anchors, both scaled by weight / avg_factor, with the dense gradients;
  * rpn_proposals: per level the top nms_pre logits (stable), decode clipped to the image, size filter on the clipped box, NMS within a level;
  * roi_loss: softmax cross-entropy and the per-class L1 with both regression targets, dense gradients, top-1 accuracy;
  * roi_predict / multiclass_nms: softmax scores, K decoded boxes per RoI, the (roi, class) candidates above score_thr, NMS within a class.
Maps are NCHW arrays (N, A * C, H, W); boxes are x1, y1, x2, y2."""
import numpy as np

import box_ref
import roi_ref
import rpn_ref

F64, F32 = np.float64, np.float32
WH_RATIO_CLIP = 16 / 1000


# ------------------------------------------------------------------------------------------------------------------- the coder
def encode(priors, gts, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), dtype=F64):
    p, g = np.asarray(priors, dtype).reshape(-1, 4), np.asarray(gts, dtype).reshape(-1, 4)
    half = dtype(0.5)
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy, gw, gh = (g[:, 0] + g[:, 2]) * half, (g[:, 1] + g[:, 3]) * half, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph)], 1)
    return ((d - np.asarray(means, dtype)) / np.asarray(stds, dtype)).astype(dtype)


def decode(priors, deltas, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), max_shape=None, wh_ratio_clip=WH_RATIO_CLIP, dtype=F64):
    """max_shape: None, one (h, w), or an (n, 2) array of per-row (h, w)"""
    p, raw = np.asarray(priors, dtype).reshape(-1, 4), np.asarray(deltas, dtype).reshape(-1, 4)
    half = dtype(0.5)
    d = raw * np.asarray(stds, dtype) + np.asarray(means, dtype)
    mr = dtype(abs(np.log(dtype(wh_ratio_clip))))
    dw, dh = np.clip(d[:, 2], -mr, mr), np.clip(d[:, 3], -mr, mr)
    px, py, pw, ph = (p[:, 0] + p[:, 2]) * half, (p[:, 1] + p[:, 3]) * half, p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy, gw, gh = px + pw * d[:, 0], py + ph * d[:, 1], pw * np.exp(dw), ph * np.exp(dh)
    out = np.stack([gx - gw * half, gy - gh * half, gx + gw * half, gy + gh * half], 1).astype(dtype)
    if max_shape is not None:
        ms = np.broadcast_to(np.asarray(max_shape, dtype).reshape(-1, 2), (len(out), 2))
        out[:, 0::2] = np.minimum(np.maximum(out[:, 0::2], dtype(0)), ms[:, 1:2])
        out[:, 1::2] = np.minimum(np.maximum(out[:, 1::2], dtype(0)), ms[:, 0:1])
    return out


# ------------------------------------------------------------------------------------------------------------------- the RPN
def rpn_loss(cls_maps, reg_maps, sizes, A, priors, gts_list, pos_list, pos_gt_list, neg_list, means, stds, cls_weight=1.0, bbox_weight=1.0, dtype=F64,
             avg_factor=None):
    """rpn_ref.loss with four deltas per anchor (reg_maps[l] (N, 4 A, H, W)), gts (K, 4) and L1: -> loss_cls (L), loss_bbox (L), dcls[l], dreg[l]
    (the gradients of the sum of all losses) and the targets of the positives per image"""
    L = len(sizes)
    cls_maps, reg_maps = [np.asarray(m, dtype) for m in cls_maps], [np.asarray(m, dtype) for m in reg_maps]
    priors = np.asarray(priors, dtype)
    avg = sum(len(p) + len(n) for p, n in zip(pos_list, neg_list)) if avg_factor is None else int(avg_factor)
    lc, lb = [np.zeros((), dtype) for _ in range(L)], [np.zeros((), dtype) for _ in range(L)]
    dcls, dreg = [np.zeros_like(m) for m in cls_maps], [np.zeros_like(m) for m in reg_maps]
    gc = dtype(cls_weight) / dtype(avg) if avg else dtype(0)
    gb = dtype(bbox_weight) / dtype(avg) if avg else dtype(0)
    targets = []
    for b, (gts, pos, pgt, neg) in enumerate(zip(gts_list, pos_list, pos_gt_list, neg_list)):
        pos, neg, pgt = np.asarray(pos, np.int64), np.asarray(neg, np.int64), np.asarray(pgt, np.int64)
        idx = np.concatenate([pos, neg])
        t = np.concatenate([np.ones(len(pos), dtype), np.zeros(len(neg), dtype)])
        lvl, y, x, a = rpn_ref.level_of(idx, sizes, A)
        tgt = encode(priors[pos], np.asarray(gts, dtype).reshape(-1, 4)[pgt], means, stds, dtype) if len(pos) else np.zeros((0, 4), dtype)
        targets.append(tgt)
        for j in range(len(idx)):
            l = int(lvl[j])
            z = cls_maps[l][b, a[j], y[j], x[j]]
            lc[l] = lc[l] + ((np.maximum(z, dtype(0)) - z * t[j]) + np.log1p(np.exp(-np.abs(z))))
            dcls[l][b, a[j], y[j], x[j]] = (dtype(1) / (dtype(1) + np.exp(-z)) - t[j]) * gc
            if j < len(pos) and pgt[j] >= 0:
                ch = a[j] * 4 + np.arange(4)
                d = reg_maps[l][b, ch, y[j], x[j]] - tgt[j]
                for c in range(4):
                    lb[l] = lb[l] + np.abs(d[c])
                dreg[l][b, ch, y[j], x[j]] = np.sign(d) * gb
    div = dtype(avg) if avg else dtype(1)
    return (np.asarray([v / div * dtype(cls_weight) for v in lc], dtype), np.asarray([v / div * dtype(bbox_weight) for v in lb], dtype), dcls, dreg, targets)


def l1_margin(pred, target):
    """the smallest |pred - target| of the L1 terms (float64): the sign of the gradient hangs on it"""
    d = np.abs(np.asarray(pred, F64) - np.asarray(target, F64))
    return float(d.min()) if d.size else np.inf


def rpn_decode_kept(cls_maps_b, reg_maps_b, priors, sizes, A, keep, means, stds, img_shape, dtype=F64):
    """the kept anchors of one image, level after level -> scores (T), boxes (T, 4) clipped to img_shape (h, w), level ids (T)"""
    firsts = np.cumsum([0] + [h * w * A for h, w in sizes])
    sc, bx, ids = [], [], []
    for l, (m, r, k) in enumerate(zip(cls_maps_b, reg_maps_b, keep)):
        z = np.transpose(np.asarray(m, dtype), (1, 2, 0)).reshape(-1)[k]
        H, W = sizes[l]
        d = np.transpose(np.asarray(r, dtype).reshape(A, 4, H, W), (2, 3, 0, 1)).reshape(-1, 4)[k]
        sc.append(dtype(1) / (dtype(1) + np.exp(-z)))
        bx.append(decode(np.asarray(priors, dtype)[firsts[l] + k], d, means, stds, img_shape, dtype=dtype))
        ids.append(np.full(len(k), l, np.int64))
    return np.concatenate(sc).astype(dtype), np.concatenate(bx), np.concatenate(ids)


def rpn_proposals(cls_maps_b, reg_maps_b, priors, sizes, A, means, stds, img_shape, nms_pre, max_per_img, iou_threshold, min_bbox_size=0, dtype=F64):
    """one image -> (keep: positions in the concatenated kept list, in output order; boxes (k, 4); scores (k); and the whole lists: scores, boxes,
    level ids, valid)"""
    keep = rpn_ref.topk_per_level(cls_maps_b, nms_pre)
    sc, bx, ids = rpn_decode_kept(cls_maps_b, reg_maps_b, priors, sizes, A, keep, means, stds, img_shape, dtype)
    valid = ((bx[:, 2] - bx[:, 0]) > dtype(min_bbox_size)) & ((bx[:, 3] - bx[:, 1]) > dtype(min_bbox_size))
    src = np.nonzero(valid)[0]
    if len(src) == 0:
        return src, bx[src], sc[src], (sc, bx, ids, valid)
    kept = src[box_ref.nms(bx[src], sc[src], iou_threshold, ids[src], dtype=dtype)][:max_per_img]
    return kept, bx[kept], sc[kept], (sc, bx, ids, valid)


# ------------------------------------------------------------------------------------------------------------------- the RoI head
def roi_loss(cls_score, bbox_pred, K, rois, gts, gt_labels, sample_gt, n_pos, n_neg, means, stds, reg_target="reference", cls_weight=1.0,
             bbox_weight=1.0, dtype=F64):
    """cls_score (B S, K + 1), bbox_pred (B S, 4 K), rois (B S, 4); sample_gt (B, S) rows of gts (G, 4); n_pos, n_neg (B).  reg_target:
    'reference' (all ones, as instance_segmentation/base_bbox_head.py passes its weights for the target) or 'encoded' (mmdet).  A positive whose
    gt row or label is out of range is padding.
    -> dict(loss_cls, loss_bbox, acc, dcls, dreg, labels (B S; -1 on padding), targets (B S, 4))"""
    z, reg = np.asarray(cls_score, dtype), np.asarray(bbox_pred, dtype)
    sample_gt = np.asarray(sample_gt)
    B, S = sample_gt.shape
    G = len(gt_labels)
    total = int(sum(min(max(int(p), 0), S) + min(max(int(n), 0), S - min(max(int(p), 0), S)) for p, n in zip(n_pos, n_neg)))
    gc = dtype(cls_weight) / dtype(max(total, 1))
    gb = dtype(bbox_weight) / dtype(total) if total else dtype(0)
    dcls, dreg = np.zeros_like(z), np.zeros_like(reg)
    labels, targets = -np.ones(B * S, np.int64), np.zeros((B * S, 4), dtype)
    lc = lb = dtype(0)
    hits = 0
    for b in range(B):
        np_ = min(max(int(n_pos[b]), 0), S)
        nn = min(max(int(n_neg[b]), 0), S - np_)
        for j in range(np_ + nn):
            r = b * S + j
            pos = j < np_
            label = K
            if pos:
                g = int(sample_gt[b, j])
                label = int(gt_labels[g]) if 0 <= g < G else -1
                if not 0 <= label < K:
                    continue
            labels[r] = label
            m = z[r].max()
            e = np.exp(z[r] - m)
            s = e.sum(dtype=dtype)
            lc = lc + ((np.log(s) + m) - z[r, label])
            hits += int(np.argmax(z[r]) == label)
            onehot = np.zeros(K + 1, dtype)
            onehot[label] = 1
            dcls[r] = (e / s - onehot) * gc
            if pos:
                t = np.ones(4, dtype) if reg_target == "reference" else encode(np.asarray(rois, dtype)[r], np.asarray(gts, dtype)[g], means, stds, dtype)[0]
                targets[r] = t
                d = reg[r, 4 * label:4 * label + 4] - t
                lb = lb + (((np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])) + np.abs(d[3]))
                dreg[r, 4 * label:4 * label + 4] = np.sign(d) * gb
    return dict(loss_cls=dtype(lc / dtype(max(total, 1)) * dtype(cls_weight)), loss_bbox=dtype(lb / dtype(total) * dtype(bbox_weight)) if total else dtype(0),
                acc=dtype(hits * 100.0 / total) if total else dtype(0), dcls=dcls, dreg=dreg, labels=labels, targets=targets)


def roi_predict(cls_score, bbox_pred, K, rois, means, stds, img_shape, inv_scale=None, wh_ratio_clip=WH_RATIO_CLIP, dtype=F64):
    """cls_score (R, K + 1), bbox_pred (R, 4 K), rois (R, 4); img_shape one (h, w) or (R, 2); inv_scale None, one (1 / sx, 1 / sy) or (R, 2)
    -> scores (R, K), boxes (R, K, 4)"""
    R = len(cls_score)
    sc = roi_ref.softmax(cls_score, dtype)[:, :K]
    p = np.repeat(np.asarray(rois, dtype).reshape(-1, 4), K, 0)
    ms = np.repeat(np.broadcast_to(np.asarray(img_shape, dtype).reshape(-1, 2), (R, 2)), K, 0)
    bx = decode(p, np.asarray(bbox_pred, dtype)[:, :4 * K].reshape(-1, 4), means, stds, ms, wh_ratio_clip, dtype)
    if inv_scale is not None:
        f = np.repeat(np.broadcast_to(np.asarray(inv_scale, dtype).reshape(-1, 2), (R, 2)), K, 0)
        bx = (bx * np.concatenate([f, f], 1)).astype(dtype)
    return sc, bx.reshape(R, K, 4)


def multiclass_nms(boxes, scores, score_thr, iou_threshold, max_per_img, dtype=F64):
    """boxes (R, K, 4), scores (R, K) of one image -> (keep: (roi, class) candidates as roi * K + class, descending score; boxes (k, 4); scores (k);
    labels (k))"""
    K = scores.shape[1]
    flat, bx = np.asarray(scores, dtype).reshape(-1), np.asarray(boxes, dtype).reshape(-1, 4)
    cand = np.nonzero(flat > dtype(score_thr))[0]
    if len(cand) == 0:
        return cand, bx[:0], flat[:0], cand
    kept = cand[box_ref.nms(bx[cand], flat[cand], iou_threshold, cand % K, dtype=dtype)]
    if max_per_img > 0:
        kept = kept[:max_per_img]
    return kept, bx[kept], flat[kept], kept % K
