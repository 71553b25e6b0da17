"""Numpy restatement of the DOTA mAP metric (Multi-Task_Pretrain/rotated_detection/metric.py: tpfp_default, get_cls_results, eval_rbbox_map) and of
mmdet's average_precision, for the tests of csrc/det_eval.hip and mtp_amd.evaluation.DOTAMetric (the sibling of box_ref.py and seg_eval_ref.py).  Plain
helper module: no tests, no fixtures.  Fixture f24 (the reference's own file, run over stubs) pins it.

The IoU comes from box_ref in `dtype` (float64 is the reference; the kernels are float32), or from `iou_fn(dets (m, 5), gts (n, 5)) -> (m, n)`.
Everything after the IoU has the reference's own dtypes: tp / fp and their cumulative sums float32, recall float64 (float32 / max(int64, float32 eps)
promotes to float64 under NumPy >= 2), precision float32, AP float32.  `prec_dtype=F64` evaluates the precisions in float64 instead: the distance of
the two area-mode APs sets the tolerance of the GPU test.

average_precision is restated from mmdet's published algorithm (mmdet is not installed).  The points that matter:
  * recalls / precisions of one scale are lifted to (1, n); `ap` is a float32 array, so every `ap[i] += prec` and the final `ap /= 11` round to float32;
  * '11points': the thresholds are np.arange(0, 1 + 1e-3, 0.1) -- i * 0.1 in float64, so 0.30000000000000004, 0.6000000000000001, 0.7000000000000001:
    a recall of exactly 3 / 10 does not reach the fourth point; prec = precisions[recalls >= thr].max(), or 0 when nothing reaches thr;
  * 'area': mrec = [0, recalls, 1], mpre = [0, precisions, 0] in recalls' dtype (float64: hstack promotes the float32 precisions), mpre made
    non-increasing from the right, then the sum over the steps `mrec[1:] != mrec[:-1]` of (mrec[i + 1] - mrec[i]) * mpre[i + 1], stored to float32.

Sorting: the reference's np.argsort(-scores) is not stable, so the order of equal scores is undefined there.  Here every sort is stable: among equal
scores the lower index goes first (inside an image: the earlier row; across images: the earlier image), which is what the kernels implement.

The threshold compare is `iou >= iou_thr` with the IoU a float32 array element and iou_thr a Python float: NumPy >= 2 compares in float32 with the
threshold rounded to float32.  The restatement compares against np.float32(iou_thr) in every dtype.
"""
import numpy as np

import box_ref as BR

F64, F32 = np.float64, np.float32
EPS32 = np.finfo(np.float32).eps
TP, FP = 1, 2      # the flag values of mtp_det_tpfp


def average_precision(recalls, precisions, mode="area"):
    no_scale = False
    if recalls.ndim == 1:
        no_scale = True
        recalls, precisions = recalls[np.newaxis, :], precisions[np.newaxis, :]
    assert recalls.shape == precisions.shape and recalls.ndim == 2
    num_scales = recalls.shape[0]
    ap = np.zeros(num_scales, dtype=np.float32)
    if mode == "area":
        zeros = np.zeros((num_scales, 1), dtype=recalls.dtype)
        ones = np.ones((num_scales, 1), dtype=recalls.dtype)
        mrec = np.hstack((zeros, recalls, ones))
        mpre = np.hstack((zeros, precisions, zeros))
        for i in range(mpre.shape[1] - 1, 0, -1):
            mpre[:, i - 1] = np.maximum(mpre[:, i - 1], mpre[:, i])
        for i in range(num_scales):
            ind = np.where(mrec[i, 1:] != mrec[i, :-1])[0]
            ap[i] = np.sum((mrec[i, ind + 1] - mrec[i, ind]) * mpre[i, ind + 1])
    elif mode == "11points":
        for i in range(num_scales):
            for thr in np.arange(0, 1 + 1e-3, 0.1):
                precs = precisions[i, recalls[i, :] >= thr]
                prec = precs.max() if precs.size > 0 else 0
                ap[i] += prec
        ap /= 11
    else:
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    if no_scale:
        ap = ap[0]
    return ap


def _iou(dets, gts, dtype, iou_fn):
    if iou_fn is not None:
        return np.asarray(iou_fn(np.asarray(dets, F32)[:, :5], np.asarray(gts, F32)))
    return BR.box_iou_rotated(np.asarray(dets)[:, :5], gts, dtype=dtype)


def tpfp_default(det_bboxes, gt_bboxes, gt_bboxes_ignore, iou_thr=0.5, dtype=F64, iou_fn=None):
    """-> (tp, fp) float32 (1, m), and ious_max (m), ious_argmax (m) into vstack(gt_bboxes, gt_bboxes_ignore) (0 / -1 without gts)"""
    det_bboxes = np.asarray(det_bboxes)
    gt_bboxes, gt_bboxes_ignore = np.asarray(gt_bboxes).reshape(-1, 5), np.asarray(gt_bboxes_ignore).reshape(-1, 5)
    gt_ignore_inds = np.concatenate((np.zeros(gt_bboxes.shape[0], dtype=bool), np.ones(gt_bboxes_ignore.shape[0], dtype=bool)))
    gt_bboxes = np.vstack((gt_bboxes, gt_bboxes_ignore))
    num_dets, num_gts = det_bboxes.shape[0], gt_bboxes.shape[0]
    tp, fp = np.zeros((1, num_dets), dtype=np.float32), np.zeros((1, num_dets), dtype=np.float32)
    if num_gts == 0:
        fp[...] = 1
        return tp, fp, np.zeros(num_dets, dtype), np.full(num_dets, -1, np.int64)
    if num_dets == 0:
        return tp, fp, np.zeros(0, dtype), np.zeros(0, np.int64)
    ious = _iou(det_bboxes, gt_bboxes, dtype, iou_fn)
    ious_max, ious_argmax = ious.max(axis=1), ious.argmax(axis=1)
    sort_inds = np.argsort(-det_bboxes[:, -1], kind="stable")
    gt_covered = np.zeros(num_gts, dtype=bool)
    for i in sort_inds:
        if ious_max[i] >= np.float32(iou_thr):
            matched_gt = ious_argmax[i]
            if not gt_ignore_inds[matched_gt]:
                if not gt_covered[matched_gt]:
                    gt_covered[matched_gt] = True
                    tp[0, i] = 1
                else:
                    fp[0, i] = 1
        else:
            fp[0, i] = 1
    return tp, fp, ious_max, ious_argmax.astype(np.int64)


def get_cls_results(det_results, annotations, class_id):
    """an image without non-ignored gts contributes no gts at all, its ignored ones included (metric.py:219-232)"""
    cls_dets = [img_res[class_id] for img_res in det_results]
    cls_gts, cls_gts_ignore = [], []
    for ann in annotations:
        if len(ann["bboxes"]) != 0:
            cls_gts.append(ann["bboxes"][ann["labels"] == class_id, :])
            cls_gts_ignore.append(ann["bboxes_ignore"][ann["labels_ignore"] == class_id, :])
        else:
            cls_gts.append(np.zeros((0, 5), dtype=np.float64))
            cls_gts_ignore.append(np.zeros((0, 5), dtype=np.float64))
    return cls_dets, cls_gts, cls_gts_ignore


def eval_rbbox_map(det_results, annotations, iou_thr=0.5, use_07_metric=True, dtype=F64, prec_dtype=F32, iou_fn=None):
    """-> (mean_ap, eval_results); each result also carries 'tp' / 'fp' (float32, score order, not cumulated) and 'tpfp' (the per-image tuples)"""
    assert len(det_results) == len(annotations)
    num_classes = len(det_results[0])
    eval_results = []
    for i in range(num_classes):
        cls_dets, cls_gts, cls_gts_ignore = get_cls_results(det_results, annotations, i)
        tpfp = [tpfp_default(d, g, gi, iou_thr, dtype, iou_fn) for d, g, gi in zip(cls_dets, cls_gts, cls_gts_ignore)]
        num_gts = np.zeros(1, dtype=int)
        for bbox in cls_gts:
            num_gts[0] += bbox.shape[0]
        dets = np.vstack(cls_dets)
        num_dets = dets.shape[0]
        sort_inds = np.argsort(-dets[:, -1], kind="stable")
        tp0 = np.hstack([t[0] for t in tpfp])[:, sort_inds]
        fp0 = np.hstack([t[1] for t in tpfp])[:, sort_inds]
        tp, fp = np.cumsum(tp0, axis=1), np.cumsum(fp0, axis=1)
        eps = np.finfo(np.float32).eps
        recalls = tp / np.maximum(num_gts[:, np.newaxis], eps)
        precisions = tp.astype(prec_dtype) / np.maximum((tp + fp).astype(prec_dtype), prec_dtype(eps))
        recalls, precisions = recalls[0, :], precisions[0, :]
        ap = average_precision(recalls, precisions, "area" if not use_07_metric else "11points")
        eval_results.append({"num_gts": num_gts.item(), "num_dets": num_dets, "recall": recalls, "precision": precisions, "ap": ap, "tp": tp0[0], "fp": fp0[0],
                             "tpfp": tpfp, "sort_inds": sort_inds})
    aps = [r["ap"] for r in eval_results if r["num_gts"] > 0]
    mean_ap = np.array(aps).mean().item() if aps else 0.0
    return mean_ap, eval_results


def compute_metrics(det_results, annotations, iou_thrs, use_07_metric=True, **kw):
    """MTP_RD_Metric.compute_metrics (metric.py:700-716): OrderedDict(mAP, AP50, ...)"""
    from collections import OrderedDict
    out, mean_aps = OrderedDict(), []
    for thr in iou_thrs:
        mean_ap, _ = eval_rbbox_map(det_results, annotations, thr, use_07_metric, **kw)
        mean_aps.append(mean_ap)
        out["AP%02d" % int(thr * 100)] = round(mean_ap, 3)
    out["mAP"] = sum(mean_aps) / len(mean_aps)
    out.move_to_end("mAP", last=False)
    return out


# ------------------------------------------------------------------------------------------------------------------- the kernels' tables
def tables(det_results, annotations):
    """the device tables of one set: detections image by image, inside an image class by class, rows in their order; gts image by image, the
    non-ignored first, then the ignored.  -> dict of numpy arrays (boxes float32)"""
    K = len(det_results[0])
    db, ds, dl, di, gb, gl, gi, start = [], [], [], [], [], [], [], [0]
    for i, (res, ann) in enumerate(zip(det_results, annotations)):
        for k in range(K):
            d = np.asarray(res[k], np.float64).reshape(-1, 6)
            db.append(d[:, :5]), ds.append(d[:, 5]), dl.append(np.full(len(d), k, np.int64)), di.append(np.full(len(d), i, np.int64))
        b, bi = np.asarray(ann["bboxes"]).reshape(-1, 5), np.asarray(ann["bboxes_ignore"]).reshape(-1, 5)
        gb += [b, bi]
        gl += [np.asarray(ann["labels"], np.int64).reshape(-1), np.asarray(ann["labels_ignore"], np.int64).reshape(-1)]
        gi += [np.zeros(len(b), np.uint8), np.ones(len(bi), np.uint8)]
        start.append(start[-1] + len(b) + len(bi))
    cat = np.concatenate
    return dict(det_boxes=cat(db).astype(F32).reshape(-1, 5), det_scores=cat(ds).astype(F32), det_labels=cat(dl), det_img=cat(di),
                gt_boxes=cat(gb).astype(F32).reshape(-1, 5), gt_labels=cat(gl), gt_ignore=cat(gi), gt_start=np.asarray(start, np.int64))


def table_results(det_results, annotations, iou_thrs, **kw):
    """what the kernels must give on tables(...): best_iou (D), best_gt (D) into the gt table, flags (T, D), num_gts (K) -- from tpfp_default per
    (class, image), put back into table order"""
    K, T = len(det_results[0]), len(iou_thrs)
    tb = tables(det_results, annotations)
    D = len(tb["det_scores"])
    best_iou, best_gt, flags, num_gts = np.zeros(D, F64), np.full(D, -1, np.int64), np.zeros((T, D), np.uint8), np.zeros(K, np.int64)
    for t, thr in enumerate(iou_thrs):
        pos = 0
        for i, (res, ann) in enumerate(zip(det_results, annotations)):
            g0 = tb["gt_start"][i]
            for k in range(K):
                cls_dets, cls_gts, cls_ign = get_cls_results([res], [ann], k)
                tp, fp, mx, arg = tpfp_default(cls_dets[0], cls_gts[0], cls_ign[0], thr, **kw)
                m = len(cls_dets[0])
                flags[t, pos:pos + m] = TP * (tp[0] > 0) + FP * (fp[0] > 0)
                if t == 0:
                    num_gts[k] += len(cls_gts[0])
                    # the class's rows of vstack(gts, ignored) -> rows of the image's part of the table
                    rows = np.concatenate([np.nonzero(np.asarray(ann["labels"]) == k)[0], len(ann["bboxes"]) + np.nonzero(np.asarray(ann["labels_ignore"]) == k)[0]])
                    best_iou[pos:pos + m] = mx
                    if len(cls_gts[0]) + len(cls_ign[0]):      # (none for an image without non-ignored gts, whatever `rows` holds)
                        best_gt[pos:pos + m] = g0 + rows[arg]
                pos += m
    return tb, best_iou, best_gt, flags, num_gts


def sorted_segments(scores, labels, K):
    """the class-major, score-descending list the AP kernel walks: order (D), cls_start (K + 1); both sorts stable"""
    o1 = np.argsort(-np.asarray(scores, F64), kind="stable")
    order = o1[np.argsort(np.asarray(labels)[o1], kind="stable")]
    counts = np.bincount(np.asarray(labels), minlength=K)[:K]
    return order.astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def ap_from_flags(flags, order, cls_start, num_gts, mode="11points", prec_dtype=F32):
    """the AP kernel's outputs from one threshold's flags (D): ap (K) float32, last_recall (K), recall (D) f64 and precision (D) by list position"""
    K = len(num_gts)
    ap, last = np.zeros(K, np.float32), np.zeros(K, F64)
    rec, prec = np.zeros(len(order), F64), np.zeros(len(order), prec_dtype)
    for k in range(K):
        s, e = cls_start[k], cls_start[k + 1]
        f = np.asarray(flags)[order[s:e]]
        tp, fp = np.cumsum((f == TP).astype(np.float32)), np.cumsum((f == FP).astype(np.float32))
        r = tp / np.maximum(np.array([num_gts[k]], dtype=int), EPS32)
        p = tp.astype(prec_dtype) / np.maximum((tp + fp).astype(prec_dtype), prec_dtype(EPS32))
        ap[k] = average_precision(r, p, mode)
        rec[s:e], prec[s:e] = r, p
        last[k] = r[-1] if e > s else 0.0
    return ap, last, rec, prec
