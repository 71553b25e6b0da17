"""CocoMetric (mmdet's CocoMetric as the reference uses it: Multi-Task_Pretrain/instance_segmentation/metric.py, MTP_IS_Metric) on the kernels of
csrc/coco_eval.hip.

The reference copies every mask to the host, RLE-encodes it, writes two json files and runs pycocotools' Python loops per (image, category, area
range).  Here `process` packs the masks to bit words, computes each image's dense (detections x gts) float64 IoU block and drops the masks -- no host
synchronisation -- and `compute_metrics` runs sort -> match -> accumulate on device tables and makes ONE host sync for one packed buffer; the twelve
statistics, the rounding and the key names are host numpy, as metric.py:493-580 and COCOeval.summarize write them.

Kept from the reference, on purpose: the gt area is the BOX area also for 'segm' (metric.py:313-321); for 'segm' a detection's area is its mask's
pixel count, for 'bbox' / 'proposal' w * h in double on the float32 corners; 'proposal' is category-agnostic and then orders an image's annotations
category by category (COCOeval gathers them per catId); images are evaluated in ascending img_id order and maxDets is sorted.  Not built, and refused
with a message: 'proposal_fast', ann_file, RLE-dict masks (their upstream code is absent); json files are written for boxes only and only with an
outfile_prefix.
"""
import json
from collections import OrderedDict

import numpy as np
import torch

from .. import ops
from ..registry import MODELS

METRIC_NAMES = {"mAP": 0, "mAP_50": 1, "mAP_75": 2, "mAP_s": 3, "mAP_m": 4, "mAP_l": 5, "AR@100": 6, "AR@300": 7, "AR@1000": 8, "AR_s@1000": 9,
                "AR_m@1000": 10, "AR_l@1000": 11}


def _get(obj, key, default=None):
    if isinstance(obj, dict):
        return obj.get(key, default)
    return getattr(obj, key, default)


def _box_area(boxes):
    """w * h in double on the float32 corners, as the json round trip of the reference computes it"""
    b = boxes.double()
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def _stable(keys, descending=False):
    return torch.sort(keys, descending=descending, stable=True)[1]


def _tables(images, kind, agnostic, num_classes):
    """the device tables of mtp_coco_match for `images` (in evaluation order), without a host sync -> dict"""
    dev, K = images[0]["scores"].device, (1 if agnostic else num_classes)
    cells = len(images) * K
    i64 = dict(dtype=torch.int64, device=dev)
    score = torch.cat([im["scores"] for im in images])
    label = torch.cat([im["labels"] for im in images])
    area = torch.cat([im["area"][kind] for im in images])
    img = torch.cat([torch.full((im["D"],), i, **i64) for i, im in enumerate(images)])
    off, rows = 0, []
    for im in images:
        rows.append(off + torch.arange(im["D"], **i64) * im["G"])
        off += im["D"] * im["G"]
    row = torch.cat(rows)
    iou = torch.cat([im["iou"][kind] for im in images])
    g_label = torch.cat([im["gt_labels"] for im in images])
    g_crowd = torch.cat([im["gt_crowd"] for im in images]).contiguous()
    g_area = torch.cat([im["gt_area"] for im in images])
    g_img = torch.cat([torch.full((im["G"],), i, **i64) for i, im in enumerate(images)])
    g_col = torch.cat([torch.arange(im["G"], **i64) for im in images]).contiguous()

    def cell_of(img, label):      # a label outside [0, num_classes) belongs to no cell and no category
        ok = (label >= 0) & (label < num_classes)
        return torch.where(ok, img * K + (torch.zeros_like(img) if agnostic else label), torch.full_like(img, cells)), torch.where(ok, torch.zeros_like(img) if agnostic else label, torch.full_like(img, K))
    cell, cat = cell_of(img, label)
    # list order, least significant key first: table order, (agnostic: category), descending score, cell -- all stable, all plumbing
    idx = torch.arange(score.shape[0], **i64)
    if agnostic:
        idx = idx[_stable(label[idx])]
    idx = idx[_stable(score[idx], descending=True)]
    idx = idx[_stable(cell[idx])]
    bounds = torch.arange(cells + 1, **i64)
    g_cell = cell_of(g_img, g_label)[0]
    g_ig = torch.stack([((g_crowd != 0) | (g_area < lo) | (g_area > hi)).to(torch.uint8) for lo, hi in ops.COCO_AREA_RNG]).contiguous()
    orders = []
    for a in range(ops.COCO_AREAS):
        g_idx = torch.arange(g_label.shape[0], **i64)
        if agnostic:
            g_idx = g_idx[_stable(g_label[g_idx])]
        g_idx = g_idx[_stable(g_ig[a][g_idx])]
        orders.append(g_idx[_stable(g_cell[g_idx])])
    g_order = torch.stack(orders).contiguous()
    return dict(iou=iou.contiguous(), det_row=row[idx].contiguous(), det_area=area[idx].contiguous(), score=score[idx].contiguous(), cat=cat[idx].contiguous(),
                det_cell_start=torch.searchsorted(cell[idx].contiguous(), bounds).contiguous(), gt_order=g_order, gt_col=g_col, gt_crowd=g_crowd, gt_ig=g_ig,
                gt_cell_start=torch.searchsorted(g_cell[g_order[0]].contiguous(), bounds).contiguous(), K=K, max_cell_gts=max(im["G"] for im in images))


def _evaluate(images, kind, agnostic, num_classes, iou_thrs, max_dets, gather=None):
    """-> precision (T, 101, K, 4, M), scores, recall (T, K, 4, M) on the device, and the per-list-position parts (score, cat, rank, matched, ignored,
    npig).  Matching is per image, so a rank matches its own images; only the parts cross the ranks."""
    if not images:      # a rank without images still takes part in the gather: empty parts
        dev, K, T = torch.device("cuda", torch.cuda.current_device()), (1 if agnostic else num_classes), len(iou_thrs)
        flags = torch.zeros(ops.COCO_AREAS, T, 0, dtype=torch.uint8, device=dev)
        parts = (torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), flags, flags.clone(),
                 torch.zeros(K, ops.COCO_AREAS, dtype=torch.int64, device=dev))
        return _accumulate(CocoMetric.merge_ranks(gather(parts)), K, max_dets)
    t = _tables(images, kind, agnostic, num_classes)
    matched, ignored, rank, npig = ops.coco_match(t["iou"], t["det_row"], t["det_area"], t["det_cell_start"], t["gt_order"], t["gt_col"], t["gt_crowd"],
                                                  t["gt_ig"], t["gt_cell_start"], t["K"], iou_thrs, max_dets[-1], max_cell_gts=t["max_cell_gts"])
    parts = (t["score"], t["cat"], rank, matched, ignored, npig)
    if gather is not None:
        parts = CocoMetric.merge_ranks(gather(parts))
    return _accumulate(parts, t["K"], max_dets)


def _accumulate(parts, K, max_dets):
    score, cat, rank, matched, ignored, npig = parts
    o1 = _stable(score, descending=True)
    sorted_cat, o2 = torch.sort(cat[o1], stable=True)
    order = o1[o2].contiguous()
    cls_start = torch.searchsorted(sorted_cat.contiguous(), torch.arange(K + 1, dtype=torch.int64, device=score.device)).contiguous()
    return ops.coco_accumulate(matched.contiguous(), ignored.contiguous(), rank.contiguous(), score.contiguous(), order, cls_start, npig, max_dets) + (parts,)


def summarize(precision, recall, iou_thrs):
    """COCOeval.summarize's twelve numbers from precision (T, R, K, A, M) / recall (T, K, A, M): means of the entries > -1 at maxDets[2] (recall also
    at maxDets[0], [1]); a threshold is found by equality with iou_thrs"""
    thrs = np.asarray(iou_thrs, np.float64)

    def one(ap, thr=None, a=0, m=2):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == thrs)[0]]
        s = s[..., a, m]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    return np.array([one(1), one(1, .5), one(1, .75), one(1, a=1), one(1, a=2), one(1, a=3), one(0, m=0), one(0, m=1), one(0), one(0, a=1), one(0, a=2),
                     one(0, a=3)], np.float64)


@MODELS.register_module(name=["CocoMetric", "MTP_IS_Metric", "mmdet.CocoMetric"])
class CocoMetric:
    """CocoMetric(ann_file=None, metric='bbox', classwise=False, proposal_nums=(100, 300, 1000), iou_thrs=None, metric_items=None, format_only=False,
    outfile_prefix=None, ..., prefix=None, classes=None, dataset_meta=None): the reference's constructor.  `gather`: None, or a callable taking this
    rank's parts (score, category, rank, matched, ignored, npig) and returning the list of every rank's parts, in rank order."""

    default_prefix = "coco"

    def __init__(self, ann_file=None, metric="bbox", classwise=False, proposal_nums=(100, 300, 1000), iou_thrs=None, metric_items=None, format_only=False,
                 outfile_prefix=None, file_client_args=None, backend_args=None, collect_device="cpu", prefix=None, sort_categories=False, classes=None,
                 dataset_meta=None):
        self.metrics = metric if isinstance(metric, list) else [metric]
        for m in self.metrics:
            if m not in ("bbox", "segm", "proposal", "proposal_fast"):
                raise KeyError(f"metric should be one of 'bbox', 'segm', 'proposal', 'proposal_fast', but got {m}.")
            if m == "proposal_fast":
                raise NotImplementedError("CocoMetric: 'proposal_fast' is not built (mmdet's eval_recalls is not part of the reference tree)")
        if ann_file is not None:
            raise NotImplementedError("CocoMetric: ann_file is not built (it needs pycocotools' COCO reader); the ground truth comes from process()")
        if file_client_args is not None:
            raise RuntimeError("The `file_client_args` is deprecated, please use `backend_args` instead")
        self.classwise, self.proposal_nums = classwise, sorted(int(n) for n in proposal_nums)
        if len(self.proposal_nums) != 3:
            raise ValueError("CocoMetric: three proposal_nums (COCOeval.summarize reads maxDets[0..2]), got %r" % (proposal_nums,))
        if iou_thrs is None:
            iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.iou_thrs = [float(t) for t in (iou_thrs if hasattr(iou_thrs, "__len__") else [iou_thrs])]
        if not 1 <= len(self.iou_thrs) <= ops.COCO_MAX_THRS:
            raise ValueError("CocoMetric: 1 to %d IoU thresholds, got %d" % (ops.COCO_MAX_THRS, len(self.iou_thrs)))
        if metric_items is not None:
            for item in metric_items:
                if item not in METRIC_NAMES:
                    raise KeyError(f'metric item "{item}" is not supported')
        self.metric_items, self.format_only, self.outfile_prefix = metric_items, format_only, outfile_prefix
        if format_only:
            assert outfile_prefix is not None, "outfile_prefix must be not None when format_only is True"
        self.prefix = self.default_prefix if prefix is None else prefix
        self.dataset_meta = dataset_meta if dataset_meta is not None else (None if classes is None else dict(classes=tuple(classes)))
        self.gather = None
        self.arrays = None      # after compute_metrics: per metric dict(precision, scores, recall, stats)
        self.reset()

    def reset(self):
        self._images, self.arrays = [], None

    @property
    def classes(self):
        if self.dataset_meta is None or "classes" not in self.dataset_meta:
            raise RuntimeError("CocoMetric: no class names -- pass classes=... or dataset_meta=dict(classes=...)")
        return tuple(self.dataset_meta["classes"])

    @property
    def num_images(self):
        return len(self._images)

    # ------------------------------------------------------------------ accumulation
    def _one(self, pred, gt, img_id):
        boxes = _get(pred, "bboxes").detach().to(torch.float32).reshape(-1, 4).contiguous()
        if not boxes.is_cuda:
            raise RuntimeError("CocoMetric.process takes device tensors (there is no CPU fallback)")
        dev, D = boxes.device, boxes.shape[0]
        scores = _get(pred, "scores").detach().to(torch.float32).reshape(-1).contiguous()
        labels = _get(pred, "labels").detach().to(torch.int64).reshape(-1).contiguous()
        assert scores.shape[0] == D and labels.shape[0] == D
        empty = gt is None or (isinstance(gt, dict) and not gt)
        gb = boxes.new_zeros(0, 4) if empty else _get(gt, "bboxes").detach().to(torch.float32).reshape(-1, 4).contiguous()
        G = gb.shape[0]
        gl = labels.new_zeros(0) if empty else _get(gt, "labels").detach().to(torch.int64).reshape(-1).contiguous()
        flag = None if empty else _get(gt, "ignore_flag")
        crowd = torch.zeros(G, dtype=torch.uint8, device=dev) if flag is None else (flag.detach().reshape(-1) != 0).to(torch.uint8).contiguous()
        if G > ops.COCO_MAX_CELL_GTS:
            raise ValueError("CocoMetric: %d gts in one image; at most %d" % (G, ops.COCO_MAX_CELL_GTS))
        im = dict(img_id=len(self._images) if img_id is None else img_id, D=D, G=G, boxes=boxes, scores=scores, labels=labels, gt_labels=gl, gt_crowd=crowd,
                  gt_area=_box_area(gb), iou={}, area={})
        # One block per kind and image.  'bbox' and 'proposal' share the box block: it is computed category-agnostic as soon as 'proposal' is
        # asked for, which changes nothing for 'bbox' (matching reads only the pairs of one cell, all of one label; the label test of the
        # kernel only saves work).  The launches are per image: mask words of different image sizes do not share a table, and every call is
        # asynchronous, so a batch costs launches, not waits.
        if "bbox" in self.metrics or "proposal" in self.metrics:
            im["iou"]["bbox"] = ops.coco_iou("bbox", boxes, labels, gb, gl, crowd, [0, D], [0, G], agnostic="proposal" in self.metrics)[0]
            im["area"]["bbox"] = _box_area(boxes)
        if "segm" in self.metrics:
            masks, gm = _get(pred, "masks"), (None if empty else _get(gt, "masks"))
            if not torch.is_tensor(masks) or (G and not torch.is_tensor(gm)):
                raise NotImplementedError("CocoMetric: 'segm' takes (n, H, W) bool mask tensors for the detections and the gts; RLE dicts and polygon "
                                          "structures are not built (their upstream code is absent)")
            scores_m = _get(pred, "mask_scores")
            if scores_m is not None:
                raise NotImplementedError("CocoMetric: mask_scores are not built")
            dw, da = ops.mask_pack(masks.detach().flatten(1).contiguous())
            if G:
                gw, ga = ops.mask_pack(gm.detach().flatten(1).contiguous())
            else:
                gw, ga = dw.new_zeros(0, dw.shape[1]), da.new_zeros(0)
            if gw.shape[1] != dw.shape[1]:
                raise ValueError("CocoMetric: detection and gt masks of different sizes")
            im["iou"]["segm"] = ops.coco_iou("segm", (dw, da), labels, (gw, ga), gl, crowd, [0, D], [0, G])[0]      # the masks and words are dropped here
            im["area"]["segm"] = da.double()
        self._images.append(im)

    def process(self, pred_instances, gt_instances=None, img_ids=None):
        """one image (dicts or objects: bboxes / scores / labels / masks, and bboxes / labels / ignore_flag / masks) or a batch (lists of them); or the
        reference's call process(data_batch, data_samples) with samples carrying pred_instances, gt_instances and img_id.  Device tensors; nothing
        here synchronises with the host."""
        samples = gt_instances
        if isinstance(samples, (list, tuple)) and not samples:
            return
        if isinstance(samples, (list, tuple)) and _get(samples[0], "pred_instances") is not None:
            for s in samples:
                if _get(s, "gt_instances") is None:
                    raise NotImplementedError("CocoMetric: a data sample needs gt_instances (device tensors); host annotation lists are not built")
                self._one(_get(s, "pred_instances"), _get(s, "gt_instances"), _get(s, "img_id"))
            return
        if isinstance(pred_instances, (list, tuple)):
            for j in range(len(pred_instances)):
                self._one(pred_instances[j], gt_instances[j], None if img_ids is None else img_ids[j])
            return
        self._one(pred_instances, gt_instances, img_ids)

    # ------------------------------------------------------------------ evaluation
    @staticmethod
    def merge_ranks(parts):
        """every rank's (score (D_r), category (D_r), rank (D_r), matched (4, T, D_r), ignored (4, T, D_r), npig (K, 4)), in rank order -> one tuple:
        detections concatenated in rank order, npig summed"""
        s, c, r, m, g, n = zip(*parts)
        return torch.cat(s), torch.cat(c), torch.cat(r), torch.cat(m, 2), torch.cat(g, 2), torch.stack(n).sum(0)

    def _ordered(self):
        if not self._images and self.gather is None:
            raise RuntimeError("CocoMetric: nothing processed yet")
        ids = [im["img_id"] for im in self._images]
        if len(set(ids)) != len(ids):
            raise ValueError("CocoMetric: duplicate img_id")
        return [self._images[i] for i in sorted(range(len(ids)), key=lambda i: ids[i])]      # COCOeval.evaluate: np.unique(imgIds)

    def compute_metrics(self, results=None):
        """-> OrderedDict with the reference's keys and rounding; `results` is accepted for the reference's signature and ignored"""
        out = OrderedDict()
        if self.outfile_prefix is not None:
            self.results2json(self.outfile_prefix)
        if self.format_only:
            return out
        images, K = self._ordered(), len(self.classes)
        if self.gather is None and sum(im["D"] for im in images) == 0:
            return out      # the reference logs 'The testing results of the whole dataset is empty.' and stops.  Under a gather hook a rank cannot
            # know that of the others and must not leave them waiting: it goes on, and a set without detections gives recall 0 / precision 0 or -1
        device, shapes = [], []
        for metric in self.metrics:
            kind, agnostic = ("segm" if metric == "segm" else "bbox"), metric == "proposal"
            pr, sc, rc, _ = _evaluate(images, kind, agnostic, K, self.iou_thrs, self.proposal_nums, self.gather)
            device += [pr.reshape(-1), sc.reshape(-1), rc.reshape(-1)]
            shapes.append((pr.shape, rc.shape))
        packed, at = torch.cat(device).cpu().numpy(), 0      # the one host sync
        self.arrays = {}
        for metric, (ps, rs) in zip(self.metrics, shapes):
            n, r = int(np.prod(ps)), int(np.prod(rs))
            pr, sc, rc = packed[at:at + n].reshape(ps), packed[at + n:at + 2 * n].reshape(ps), packed[at + 2 * n:at + 2 * n + r].reshape(rs)
            at += 2 * n + r
            stats = summarize(pr, rc, self.iou_thrs)
            self.arrays[metric] = dict(precision=pr, scores=sc, recall=rc, stats=stats)
            if metric == "proposal":
                for item in self.metric_items or ["AR@100", "AR@300", "AR@1000", "AR_s@1000", "AR_m@1000", "AR_l@1000"]:
                    out[item] = float(f"{stats[METRIC_NAMES[item]]:.3f}")
                continue
            if self.classwise:
                for idx, name in enumerate(self.classes):
                    p = pr[:, :, idx, 0, -1]
                    p = p[p > -1]
                    out[f"{name}_precision"] = round(np.mean(p) if p.size else float("nan"), 3)
            for item in self.metric_items or ["mAP", "mAP_50", "mAP_75", "mAP_s", "mAP_m", "mAP_l"]:
                out[f"{metric}_{item}"] = float(f"{round(stats[METRIC_NAMES[item]], 3)}")
        return out

    def evaluate(self, size=None):
        """mmengine's BaseMetric.evaluate: the metrics under '<prefix>/', then reset"""
        m = self.compute_metrics()
        self.reset()
        return {("%s/%s" % (self.prefix, k)) if self.prefix else k: v for k, v in m.items()}

    def results2json(self, outfile_prefix):
        """the box list of metric.py:225-261 -> '<outfile_prefix>.bbox.json' (host code: one transfer per image)"""
        rows = []
        for im in self._images:
            b, s, l = im["boxes"].cpu().numpy(), im["scores"].cpu().numpy(), im["labels"].cpu().numpy()
            for i, label in enumerate(l):
                bb = b[i].tolist()
                rows.append(dict(image_id=im["img_id"], bbox=[bb[0], bb[1], bb[2] - bb[0], bb[3] - bb[1]], score=float(s[i]), category_id=int(label)))
        files = dict(bbox=f"{outfile_prefix}.bbox.json", proposal=f"{outfile_prefix}.bbox.json")
        with open(files["bbox"], "w") as f:
            json.dump(rows, f)
        return files


def eval_coco(preds, gts, num_classes, metric="bbox", iou_thrs=None, proposal_nums=(100, 300, 1000), img_ids=None):
    """the functional form: preds / gts lists over the images (as CocoMetric.process takes them) -> dict(precision, scores, recall, stats) of full
    numpy arrays, and `parts`: the per-list-position (score, category, rank, matched, ignored, npig) as numpy"""
    m = CocoMetric(metric=metric, iou_thrs=iou_thrs, proposal_nums=proposal_nums, classes=["c%d" % k for k in range(num_classes)])
    m.process(list(preds), list(gts), img_ids)
    kind, agnostic = ("segm" if metric == "segm" else "bbox"), metric == "proposal"
    pr, sc, rc, parts = _evaluate(m._ordered(), kind, agnostic, num_classes, m.iou_thrs, m.proposal_nums)
    pr, sc, rc = pr.cpu().numpy(), sc.cpu().numpy(), rc.cpu().numpy()
    return dict(precision=pr, scores=sc, recall=rc, stats=summarize(pr, rc, m.iou_thrs), parts=tuple(p.cpu().numpy() for p in parts))
