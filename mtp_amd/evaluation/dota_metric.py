"""DOTAMetric (mmrotate's DOTAMetric as the reference uses it: Multi-Task_Pretrain/rotated_detection/metric.py, MTP_RD_Metric) on the kernels of
csrc/det_eval.hip.

The reference moves every image's predictions to the host, and for every class and image calls box_iou_rotated once and loops over the detections in
Python (tpfp_default).  Here `process` only appends device tensors to the detection and gt tables -- no host synchronisation -- and `compute_metrics`
runs three launches whatever the number of images and classes (match, tp / fp flags, AP) between two device sorts, then makes the ONE host sync, for
the (T, K) AP table and the per-class counts.  The mean over the classes with gts, the rounding and the key order are the reference's own host
expressions (metric.py:374-378, 700-716).

Kept from the reference, on purpose: the threshold compare in float32 (NumPy >= 2 rounds the Python-float threshold to the float32 of the IoU), the
eleven recall points of np.arange(0, 1 + 1e-3, 0.1), and get_cls_results' rule that an image without non-ignored gts has no gts at all, its ignored
ones included.  Different, on purpose: the reference's np.argsort(-scores) is not stable, so equal scores are ordered arbitrarily there; here the
earlier detection goes first (stable sorts, and the lower index wins a gt among equal scores).  The reference writes a COCO-style json in every
compute_metrics (to a temporary directory when no prefix is given); here only with an outfile_prefix.
"""
import json
import os
import os.path as osp
import re
import zipfile
from collections import OrderedDict

import numpy as np
import torch

from .. import ops
from ..registry import MODELS


def rbox2qbox(boxes):
    """mmrotate's rbox2qbox: (n, 5) cx, cy, w, h, theta -> (n, 8) x1, y1, ..., x4, y4.  With u = w / 2 (cos, sin) and v = h / 2 (-sin, cos) the corners
    are centre + u + v, centre + u - v, centre - u - v, centre - u + v, in this order."""
    ctr, w, h, theta = torch.split(boxes, (2, 1, 1, 1), dim=-1)
    cos_value, sin_value = torch.cos(theta), torch.sin(theta)
    vec1 = torch.cat([w / 2 * cos_value, w / 2 * sin_value], dim=-1)
    vec2 = torch.cat([-h / 2 * sin_value, h / 2 * cos_value], dim=-1)
    return torch.cat([ctr + vec1 + vec2, ctr + vec1 - vec2, ctr - vec1 - vec2, ctr - vec1 + vec2], dim=-1)


def _get(obj, key):
    return obj[key] if isinstance(obj, dict) else getattr(obj, key)


def _mean_ap(ap, num_gts):
    """the reference's expression (metric.py:374-378) on one threshold's float32 APs"""
    aps = [a for a, n in zip(ap, num_gts) if n > 0]
    return np.array(aps).mean().item() if aps else 0.0


def _evaluate(tables, num_classes, iou_thrs, mode, curves=False, gather=None):
    """the device part: tables = (det_boxes, det_scores, det_labels, det_img, gt_boxes, gt_labels, gt_ignore, gt_start) of this rank.  Matching is
    per image, so a rank matches its own images; only (scores, labels, flags, num_gts) cross the ranks.  -> ops.det_ap's outputs and num_gts"""
    det_boxes, det_scores, det_labels, det_img, gt_boxes, gt_labels, gt_ignore, gt_start = tables
    D, T, dev = det_boxes.shape[0], len(iou_thrs), det_boxes.device
    if D:
        best_iou, best_gt, winner = ops.det_match(det_boxes, det_scores, det_labels, det_img, gt_boxes, gt_labels, gt_ignore, gt_start, iou_thrs)
        flags, num_gts = ops.det_tpfp(det_scores, best_iou, best_gt, gt_labels, gt_ignore, iou_thrs, winner, num_classes)
    else:
        flags = torch.zeros(T, 0, dtype=torch.uint8, device=dev)
        keep = (gt_ignore == 0) & (gt_labels >= 0) & (gt_labels < num_classes)
        num_gts = torch.zeros(num_classes, dtype=torch.int64, device=dev).index_add_(0, gt_labels[keep], torch.ones_like(gt_labels[keep]))
    if gather is not None:
        det_scores, det_labels, flags, num_gts = DOTAMetric.merge_ranks(gather((det_scores, det_labels, flags, num_gts)))
    # sorting is plumbing: stable by descending score, then stable by label -> the class-major list and its offsets, no host sync
    o1 = torch.sort(det_scores, descending=True, stable=True)[1]
    sorted_labels, o2 = torch.sort(det_labels[o1], stable=True)
    order = o1[o2].contiguous()
    cls_start = torch.searchsorted(sorted_labels, torch.arange(num_classes + 1, device=dev, dtype=torch.int64)).contiguous()
    return ops.det_ap(flags.contiguous(), order, cls_start, num_gts, mode, curves) + (num_gts, order, cls_start)


@MODELS.register_module(name=["DOTAMetric", "MTP_RD_Metric", "mmrotate.DOTAMetric"])
class DOTAMetric:
    """DOTAMetric(iou_thrs=0.5, scale_ranges=None, metric='mAP', predict_box_type='rbox', format_only=False, outfile_prefix=None, merge_patches=False,
    iou_thr=0.1, eval_mode='11points', prefix=None, classes=None, dataset_meta=None).  The class names come from `classes` or
    dataset_meta['classes'] (which a runner may also set after construction).  `gather`: None, or a callable taking this rank's (scores, labels,
    flags, num_gts) and returning the list of every rank's tuples, in rank order (a test hook; with torch.distributed up and more than one rank it is
    an all-gather).  At most ops.DET_MAX_THRS thresholds and ops.DET_MAX_CLASSES classes."""

    default_prefix = "dota"

    def __init__(self, iou_thrs=0.5, scale_ranges=None, metric="mAP", predict_box_type="rbox", format_only=False, outfile_prefix=None,
                 merge_patches=False, iou_thr=0.1, eval_mode="11points", collect_device="cpu", prefix=None, nproc=1, classes=None, dataset_meta=None):
        self.iou_thrs = [float(iou_thrs)] if isinstance(iou_thrs, (float, int)) else list(iou_thrs)
        assert isinstance(self.iou_thrs, list)
        if not 1 <= len(self.iou_thrs) <= ops.DET_MAX_THRS:
            raise ValueError("DOTAMetric: 1 to %d IoU thresholds, got %d" % (ops.DET_MAX_THRS, len(self.iou_thrs)))
        if scale_ranges is not None:
            raise NotImplementedError("DOTAMetric: scale_ranges is not built (the reference itself raises NotImplementedError for area ranges as soon "
                                      "as an image has a gt, metric.py:164-167)")
        if not isinstance(metric, str):
            assert len(metric) == 1
            metric = metric[0]
        if metric not in ["mAP"]:
            raise KeyError(f"metric should be one of 'mAP', but got {metric}.")
        if predict_box_type != "rbox":
            raise NotImplementedError("DOTAMetric: predict_box_type %r is not built; only 'rbox' (cx, cy, w, h, theta) is" % (predict_box_type,))
        if eval_mode not in ops.DET_AP_MODE:
            raise ValueError("DOTAMetric: eval_mode must be '11points' or 'area', got %r" % (eval_mode,))
        if format_only:
            assert outfile_prefix is not None, "outfile_prefix must be not None when format_only is True"
        self.scale_ranges, self.metric, self.predict_box_type = None, metric, predict_box_type
        self.format_only, self.outfile_prefix, self.merge_patches, self.iou_thr = format_only, outfile_prefix, merge_patches, float(iou_thr)
        self.eval_mode, self.use_07_metric = eval_mode, eval_mode == "11points"
        self.prefix = self.default_prefix if prefix is None else prefix
        self.dataset_meta = dataset_meta if dataset_meta is not None else (None if classes is None else dict(classes=tuple(classes)))
        self.gather = None
        self.per_class = None      # after compute_metrics: num_gts (K), num_dets (K), recall (T, K), ap (T, K)
        self.reset()

    # ------------------------------------------------------------------ accumulation
    def reset(self):
        self._dets, self._gts, self._gt_counts, self._img_ids = [], [], [], []
        self.per_class = None

    @property
    def classes(self):
        if self.dataset_meta is None or "classes" not in self.dataset_meta:
            raise RuntimeError("DOTAMetric: no class names -- pass classes=... or dataset_meta=dict(classes=...)")
        return tuple(self.dataset_meta["classes"])

    @property
    def num_images(self):
        return len(self._img_ids)

    def _one(self, pred, gt, ignored, img_id):
        boxes = _get(pred, "bboxes").detach().to(torch.float32).reshape(-1, 5)
        if not boxes.is_cuda:
            raise RuntimeError("DOTAMetric.process takes device tensors (there is no CPU fallback)")
        dev, m, i = boxes.device, boxes.shape[0], len(self._img_ids)
        scores = _get(pred, "scores").detach().to(torch.float32).reshape(-1)
        labels = _get(pred, "labels").detach().to(torch.int64).reshape(-1)
        assert scores.shape[0] == m and labels.shape[0] == m
        self._dets.append((boxes, scores, labels, torch.full((m,), i, dtype=torch.int64, device=dev)))
        empty = gt is None or (isinstance(gt, dict) and not gt)
        gb = boxes.new_zeros(0, 5) if empty else _get(gt, "bboxes").detach().to(torch.float32).reshape(-1, 5)
        gl = labels.new_zeros(0) if empty else _get(gt, "labels").detach().to(torch.int64).reshape(-1)
        none = empty or ignored is None or (isinstance(ignored, dict) and not ignored)
        ib = boxes.new_zeros(0, 5) if none else _get(ignored, "bboxes").detach().to(torch.float32).reshape(-1, 5)
        il = labels.new_zeros(0) if none else _get(ignored, "labels").detach().to(torch.int64).reshape(-1)
        n, ni = gb.shape[0], ib.shape[0]
        flag = torch.cat([torch.zeros(n, dtype=torch.uint8, device=dev), torch.ones(ni, dtype=torch.uint8, device=dev)])
        self._gts.append((torch.cat([gb, ib]), torch.cat([gl, il]), flag))      # the reference's stacking order: np.vstack((gts, ignored))
        self._gt_counts.append(torch.full((1,), n + ni, dtype=torch.int64, device=dev))      # (a fill, not a host copy)
        self._img_ids.append(i if img_id is None else img_id)

    def process(self, pred_instances, gt_instances=None, ignored_instances=None, img_ids=None):
        """one image (dicts or objects with bboxes / scores / labels, bboxes / labels, bboxes / labels of the ignored gts) or a batch (lists of
        them); or the reference's call process(data_batch, data_samples) with samples carrying r_pred_instances / r_gt_instances /
        r_ignored_instances / img_id.  Device tensors; nothing here synchronises with the host."""
        samples = gt_instances
        if isinstance(samples, (list, tuple)) and not samples:
            return      # an empty batch
        if isinstance(samples, (list, tuple)) and (hasattr(samples[0], "r_pred_instances") or (isinstance(samples[0], dict) and "r_pred_instances" in samples[0])):
            for s in samples:
                ids = _get(s, "img_id") if (hasattr(s, "img_id") or (isinstance(s, dict) and "img_id" in s)) else None
                self._one(_get(s, "r_pred_instances"), _get(s, "r_gt_instances"), _get(s, "r_ignored_instances"), ids)
            return
        if isinstance(pred_instances, (list, tuple)):
            n = len(pred_instances)
            for j in range(n):
                self._one(pred_instances[j], gt_instances[j], None if ignored_instances is None else ignored_instances[j], None if img_ids is None else img_ids[j])
            return
        self._one(pred_instances, gt_instances, ignored_instances, img_ids)

    def tables(self):
        """(det_boxes (D, 5), det_scores (D), det_labels (D), det_img (D), gt_boxes (G, 5), gt_labels (G), gt_ignore (G), gt_start (I + 1)) on the
        device, without a host sync"""
        if not self._img_ids:
            raise RuntimeError("DOTAMetric: nothing processed yet")
        det = [torch.cat(c).contiguous() for c in zip(*self._dets)]
        gt = [torch.cat(c).contiguous() for c in zip(*self._gts)]
        counts = torch.cat(self._gt_counts)
        return tuple(det) + tuple(gt) + (torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).contiguous(),)

    # ------------------------------------------------------------------ evaluation
    @staticmethod
    def merge_ranks(parts):
        """parts: every rank's (scores (D_r), labels (D_r), flags (T, D_r), num_gts (K)), in rank order -> one tuple: detections concatenated in
        rank order (so that equal scores keep the order of a single rank that saw the images in the same order), num_gts summed"""
        s, l, f, n = zip(*parts)
        return torch.cat(s), torch.cat(l), torch.cat(f, 1), torch.stack(n).sum(0)

    def _gather_fn(self):
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            def all_gather(part):
                """sizes differ between the ranks: the counts go first (a host sync of its own, in the distributed path only), then padded tensors"""
                world, (s, l, f, n) = dist.get_world_size(), part
                sizes = [torch.zeros(1, dtype=torch.int64, device=s.device) for _ in range(world)]
                dist.all_gather(sizes, torch.full((1,), s.shape[0], dtype=torch.int64, device=s.device))
                sizes = [int(v) for v in torch.cat(sizes).tolist()]
                top, out = max(sizes), [[] for _ in range(world)]
                for t, dim in ((s, 0), (l, 0), (f, 1)):
                    pad = list(t.shape)
                    pad[dim] = top - t.shape[dim]
                    mine = torch.cat([t, t.new_zeros(pad)], dim).contiguous()
                    got = [torch.empty_like(mine) for _ in range(world)]
                    dist.all_gather(got, mine)
                    for r in range(world):
                        out[r].append(got[r].narrow(dim, 0, sizes[r]))
                got = [torch.empty_like(n) for _ in range(world)]
                dist.all_gather(got, n.contiguous())
                return [tuple(out[r]) + (got[r],) for r in range(world)]
            return all_gather
        return self.gather

    def compute_metrics(self, results=None):
        """-> OrderedDict(mAP=..., AP50=..., ...) with the reference's keys, rounding and order; empty after merge_patches / format_only, which write
        their files instead.  `results` is accepted for the reference's signature and ignored: the tables are the state."""
        out = OrderedDict()
        if self.merge_patches:
            self.merge_results(self.outfile_prefix)
            return out
        if self.outfile_prefix is not None:
            self.results2json(self.outfile_prefix)
        if self.format_only:
            return out
        K, T = len(self.classes), len(self.iou_thrs)
        ap, num_dets, last_recall, _, _, num_gts, _, _ = _evaluate(self.tables(), K, self.iou_thrs, self.eval_mode, gather=self._gather_fn())
        packed = torch.cat([ap.double().reshape(-1), last_recall.reshape(-1), num_gts.double(), num_dets.double()]).cpu().numpy()      # the one host sync
        ap = packed[:T * K].astype(np.float32).reshape(T, K)
        recall = packed[T * K:2 * T * K].reshape(T, K)
        num_gts, num_dets = packed[2 * T * K:2 * T * K + K].astype(np.int64), packed[2 * T * K + K:].astype(np.int64)
        self.per_class = dict(num_gts=num_gts, num_dets=num_dets, recall=recall, ap=ap)
        mean_aps = []
        for t, iou_thr in enumerate(self.iou_thrs):
            mean_ap = _mean_ap(ap[t], num_gts)
            mean_aps.append(mean_ap)
            out[f"AP{int(iou_thr * 100):02d}"] = round(mean_ap, 3)
        out["mAP"] = sum(mean_aps) / len(mean_aps)
        out.move_to_end("mAP", last=False)
        return out

    def evaluate(self, size=None):
        """mmengine's BaseMetric.evaluate: the metrics under '<prefix>/', then reset"""
        m = self.compute_metrics()
        self.reset()
        return {("%s/%s" % (self.prefix, k)) if self.prefix else k: v for k, v in m.items()}

    # ------------------------------------------------------------------ files
    def results2json(self, outfile_prefix):
        """the COCO-style list of metric.py:580-619 -> '<outfile_prefix>.bbox.json' (host code: one transfer per image)"""
        rows = []
        for img_id, (boxes, scores, labels, _) in zip(self._img_ids, self._dets):
            b, s, l = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
            for i, label in enumerate(l):
                rows.append(dict(image_id=img_id, bbox=b[i].tolist(), score=float(s[i]), category_id=int(label)))
        files = dict(bbox=f"{outfile_prefix}.bbox.json")
        with open(files["bbox"], "w") as f:
            json.dump(rows, f)
        return files

    def merged_detections(self):
        """patch ids 'name__W__x___y' -> the detections moved by (x, y) into their original image, then NMS per (original image, class) in ONE call
        of the grouped rotated NMS at iou_thr (group id = image * K + class).  -> (names, image index (k), labels (k), boxes (k, 5), scores (k)) of
        the kept ones on the host, by descending score.  At most ops.NMS_MAX_BOXES detections."""
        names, index, shift = [], [], []
        for img_id in self._img_ids:
            img_id = str(img_id)
            oriname = img_id.split("__")[0]
            x_y = re.findall(r"__\d+___\d+", img_id)
            if not x_y:
                raise ValueError("DOTAMetric.merge_results: image id %r is not of the form name__W__x___y" % (img_id,))
            x, y = (int(v) for v in re.findall(r"\d+", x_y[0])[:2])
            if oriname not in names:
                names.append(oriname)
            index.append(names.index(oriname))
            shift.append((x, y))
        boxes, scores, labels, img = (torch.cat(c) for c in zip(*self._dets))
        K, dev = len(self.classes), boxes.device
        empty = np.zeros(0, np.int64)
        if boxes.shape[0] == 0:
            return names, empty, empty, np.zeros((0, 5), np.float32), np.zeros(0, np.float32)
        ops.check_nms_count(boxes.shape[0])
        orig = torch.tensor(index, dtype=torch.int64, device=dev)[img]
        moved = boxes.clone()
        moved[:, :2] += torch.tensor(shift, dtype=torch.float32, device=dev)[img]
        order = torch.sort(scores, descending=True, stable=True)[1]
        groups = (orig * K + labels)[order].contiguous()
        keep, count = ops.nms_sorted(moved[order].contiguous(), self.iou_thr, groups, rotated=True)
        kept = order[keep[:int(count.item())]]
        packed = torch.cat([moved[kept].double(), scores[kept, None].double(), labels[kept, None].double(), orig[kept, None].double()], 1).cpu().numpy()
        return names, packed[:, 7].astype(np.int64), packed[:, 6].astype(np.int64), packed[:, :5].astype(np.float32), packed[:, 5].astype(np.float32)

    def merge_results(self, outfile_prefix):
        """merged_detections, then write_task1 -> the zip's path"""
        if outfile_prefix is None:
            raise ValueError("DOTAMetric.merge_results needs an outfile_prefix")
        return self.write_task1(outfile_prefix, self.classes, *self.merged_detections())

    @staticmethod
    def write_task1(outfile_prefix, classes, names, orig, labels, boxes, scores):
        """Task1_<class>.txt (image name, round(score, 2), eight '%.2f' corner coordinates per line) and '<prefix>/<last part>.zip', as
        metric.py:541-578 writes them -> the zip's path.  Host code: names = the original images, orig / labels / boxes (k, 5) float32 / scores the
        kept detections, inside an (image, class) by descending score."""
        if osp.exists(outfile_prefix):
            raise ValueError(f"The outfile_prefix should be a non-exist path, but {outfile_prefix} is existing. Please delete it firstly.")
        os.makedirs(outfile_prefix)
        files = [osp.join(outfile_prefix, "Task1_" + cls + ".txt") for cls in classes]
        # the reference's arrays are float64 here (labels, boxes and scores were concatenated into one array): so are the corners
        qboxes = rbox2qbox(torch.from_numpy(np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 5)))
        for k, path in enumerate(files):
            with open(path, "w") as f:
                for n, name in enumerate(names):
                    for j in np.nonzero((orig == n) & (labels == k))[0]:      # ascending j: descending score
                        f.write(" ".join([name, str(round(float(scores[j]), 2))] + [f"{p:.2f}" for p in qboxes[j]]) + "\n")
        zip_path = osp.join(outfile_prefix, osp.split(outfile_prefix)[-1] + ".zip")
        with zipfile.ZipFile(zip_path, "w", zipfile.ZIP_DEFLATED) as t:
            for f in files:
                t.write(f, osp.split(f)[-1])
        return zip_path


def eval_rbbox_map(det_results, annotations, scale_ranges=None, iou_thr=0.5, use_07_metric=True, box_type="rbox", dataset=None, logger=None, nproc=4,
                   device=None):
    """the reference's functional form (metric.py:236-383): det_results[image][class] (m, 6) arrays, annotations[image] = dict(bboxes (n, 5), labels
    (n), bboxes_ignore, labels_ignore) -> (mean_ap, [dict(num_gts, num_dets, recall, precision, ap) per class]) with the full recall (float64) and
    precision (float32) arrays.  The lists go to the device once, the results come back once."""
    if scale_ranges is not None:
        raise NotImplementedError("eval_rbbox_map: scale_ranges is not built (the reference raises NotImplementedError for area ranges itself)")
    if box_type != "rbox":
        raise NotImplementedError("eval_rbbox_map: box_type %r is not built; only 'rbox' is" % (box_type,))
    assert len(det_results) == len(annotations)
    K = len(det_results[0])
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    a = lambda v, dt: np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dt)      # noqa: E731
    db, dl, di, gb, gl, gi, start = [], [], [], [], [], [], [0]
    for i, (res, ann) in enumerate(zip(det_results, annotations)):
        for k in range(K):
            d = a(res[k], np.float32).reshape(-1, 6)
            db.append(d), dl.append(np.full(len(d), k, np.int64)), di.append(np.full(len(d), i, np.int64))
        b = a(ann["bboxes"], np.float32).reshape(-1, 5) if len(ann) else np.zeros((0, 5), np.float32)
        bi = a(ann.get("bboxes_ignore", np.zeros((0, 5))), np.float32).reshape(-1, 5) if len(b) else np.zeros((0, 5), np.float32)
        gb += [b, bi]
        gl += [a(ann["labels"], np.int64).reshape(-1) if len(b) else np.zeros(0, np.int64), a(ann.get("labels_ignore", np.zeros(0)), np.int64).reshape(-1)[:len(bi)]]
        gi += [np.zeros(len(b), np.uint8), np.ones(len(bi), np.uint8)]
        start.append(start[-1] + len(b) + len(bi))
    d = np.concatenate(db)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)      # noqa: E731
    tables = (t(d[:, :5]), t(d[:, 5]), t(np.concatenate(dl)), t(np.concatenate(di)), t(np.concatenate(gb)), t(np.concatenate(gl)), t(np.concatenate(gi)),
              t(np.asarray(start, np.int64)))
    ap, num_dets, _, recall, precision, num_gts, _, cls_start = _evaluate(tables, K, [float(iou_thr)], "11points" if use_07_metric else "area", curves=True)
    ap, num_dets, num_gts, cls_start = ap.cpu().numpy()[0], num_dets.cpu().numpy(), num_gts.cpu().numpy(), cls_start.cpu().numpy()
    recall, precision = recall.cpu().numpy()[0], precision.cpu().numpy()[0]
    results = [dict(num_gts=int(num_gts[k]), num_dets=int(num_dets[k]), recall=recall[cls_start[k]:cls_start[k + 1]],
                    precision=precision[cls_start[k]:cls_start[k + 1]], ap=ap[k]) for k in range(K)]
    return _mean_ap(ap, num_gts), results
