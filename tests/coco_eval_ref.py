"""numpy restatement of the COCO detection evaluation that the reference's instance-segmentation metric delegates to (Multi-Task_Pretrain/
instance_segmentation/metric.py: MTP_IS_Metric = mmdet's CocoMetric -> pycocotools' COCO.loadRes and COCOeval.evaluate / accumulate / summarize, and
maskApi.c's bbIou / rleIou behind computeIoU).  pycocotools is neither in the reference tree nor installed: this file is written from the published
algorithm and is UNPINNED -- nothing here was compared with the upstream code by running it.  Fixture f27 (tests/golden/make_coco_metric.py, which
runs the reference's metric.py over stubs with this file in the place of pycocotools) pins the reference's OWN code around it (process, gt_to_coco_json, results2json, the json round trip, params, key names, rounding); the kernels of
csrc/coco_eval.hip are tested against this file.  Every rule, for a reader who compares with cocoeval.py / coco.py / maskApi.c:

 loadRes      detections with a 'bbox': area = w * h, iscrowd = 0, id = position + 1.  Without (the reference pops 'bbox' for 'segm'): area = the mask's
              pixel count.  An empty list raises IndexError (anns[0]).
 _prepare     gt 'ignore' = iscrowd.  Annotations are gathered image by image in annotation order and binned by (image, category).
 evaluate     imgIds and (with useCats) catIds pass through np.unique (sorted); maxDets is sorted; without useCats one category -1 holds every
              annotation of p.catIds, GROUPED BY CATEGORY in catIds order (the comprehension runs over catIds first).
 computeIoU   detections sorted by -score with mergesort (stable), the first maxDets[-1] kept; [] when either side is empty.
   bbox       on x, y, w, h doubles: w = fmin(dw + dx, gw + gx) - fmax(dx, gx), h likewise; 0 unless w > 0 and h > 0; i = w h;
              u = crowd ? da : da + ga - i; i / u.
   segm       i = pixels set in both; u = crowd ? a_d : a_d + a_g - i; (double) i / (double) u; 0 when i = 0 (upstream never divides then: disjoint
              bounding boxes skip the run-length walk, and a walk with i = 0 gives 0 / u).
 evaluateImg  per area range [lo, hi], both ends inclusive: gt _ignore = ignore or area < lo or area > hi; gts sorted by _ignore with mergesort;
              detections by -score with mergesort, the first maxDet.  Per threshold t, per detection in order: iou = min(t, 1 - 1e-10), m = -1; walk
              the gts: skip a matched non-crowd gt; stop at the first ignored gt once a non-ignored one is held; skip when ious[d, g] < iou; else
              hold it (iou = ious[d, g], m = g) -- so among equal IoUs the LATER gt wins.  A match records dtIg = gtIg[m], dtm = the gt's id (ids
              start at 1), gtm.  Afterwards an UNMATCHED detection whose own area lies outside [lo, hi] is ignored.  None when the cell has neither
              gts nor detections.
 accumulate   per (category, area range, maxDet): the cells' first maxDet detections concatenated in image order, sorted by -score with mergesort;
              npig = the gts with gtIg == 0; npig == 0 (or no cell at all) leaves -1.  tp = cumsum(dtm != 0 & !dtIg), fp = cumsum(dtm == 0 & !dtIg);
              rc = tp / npig, pr = tp / (fp + tp + np.spacing(1)); recall = rc[-1] (0 without detections); pr made non-increasing from the right;
              inds = searchsorted(rc, recThrs, 'left'); precision[r] = pr[inds[r]], scores[r] = the sorted score there; the loop stops at the first
              index past the end and leaves the zeros.
 summarize    mean of the entries > -1 (-1 when none): stats[0..2] precision at all t / t == .5 / t == .75, area 'all', maxDets[2]; [3..5] small,
              medium, large; [6..8] recall at maxDets[0..2], area 'all'; [9..11] recall small, medium, large at maxDets[2].  A threshold is found by
              iouThr == p.iouThrs (none: -1).
"""
import copy
import json
from collections import defaultdict

import numpy as np

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


# ---------------------------------------------------------------------------------------------------------------- masks
def encode_masks(masks):
    """a lossless, json-able stand-in for the run-length encoding: (n, H, W) bool -> [dict(size=[H, W], counts=hex of np.packbits)]"""
    masks = np.asarray(masks).astype(bool)
    return [dict(size=[int(m.shape[0]), int(m.shape[1])], counts=np.packbits(m.reshape(-1)).tobytes().hex()) for m in masks]


def decode_mask(seg):
    h, w = seg["size"]
    return np.unpackbits(np.frombuffer(bytes.fromhex(seg["counts"]), np.uint8))[:h * w].astype(bool)


def mask_pack(masks):
    """(n, ...) bool -> words (n, ceil(HW / 64)) uint64 with bit p of word w = pixel 64 w + p, and the pixel counts (n) int64"""
    m = np.asarray(masks).astype(bool).reshape(len(masks), -1)
    n, hw = m.shape
    W = (hw + 63) // 64
    pad = np.zeros((n, W * 64), np.uint8)
    pad[:, :hw] = m
    words = np.packbits(pad.reshape(n, W, 8, 8), axis=-1, bitorder="little").reshape(n, W, 8).copy().view("<u8").reshape(n, W)
    return words, m.sum(1).astype(np.int64)


def mask_iou(dm, gm, crowd):
    """dm (D, HW) / gm (G, HW) bool -> iou (D, G) float64, intersections (D, G) int64"""
    dm, gm = np.asarray(dm).astype(np.int64), np.asarray(gm).astype(np.int64)
    inter = dm @ gm.T if len(dm) and len(gm) else np.zeros((len(dm), len(gm)), np.int64)
    ad, ag = dm.sum(1), gm.sum(1)
    out = np.zeros(inter.shape, np.float64)
    for d in range(inter.shape[0]):
        for g in range(inter.shape[1]):
            i = int(inter[d, g])
            if i > 0:
                u = int(ad[d]) if crowd[g] else int(ad[d]) + int(ag[g]) - i
                out[d, g] = np.float64(i) / np.float64(u)
    return out, inter


def bbox_iou(dt, gt, crowd):
    """maskApi.c bbIou: dt (D, 4) / gt (G, 4) x, y, w, h float64 -> (D, G) float64"""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    out = np.zeros((len(dt), len(gt)), np.float64)
    for g in range(len(gt)):
        G = gt[g]
        ga = G[2] * G[3]
        for d in range(len(dt)):
            D = dt[d]
            da = D[2] * D[3]
            w = np.fmin(D[2] + D[0], G[2] + G[0]) - np.fmax(D[0], G[0])
            if w <= 0:
                continue
            h = np.fmin(D[3] + D[1], G[3] + G[1]) - np.fmax(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd[g] else da + ga - i
            out[d, g] = i / u
    return out


# ---------------------------------------------------------------------------------------------------------------- COCO
class COCO:
    """coco.py's index over a dataset dict (or the path of its json), with the snake_case names mmdet's wrapper adds"""

    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = dict(), dict(), dict(), dict()
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        if annotation_file is not None:
            if isinstance(annotation_file, dict):
                self.dataset = annotation_file
            else:
                with open(annotation_file) as f:
                    self.dataset = json.load(f)
            self.createIndex()

    def createIndex(self):
        anns, cats, imgs = {}, {}, {}
        imgToAnns, catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get("annotations", []):
            imgToAnns[ann["image_id"]].append(ann)
            anns[ann["id"]] = ann
        for img in self.dataset.get("images", []):
            imgs[img["id"]] = img
        for cat in self.dataset.get("categories", []):
            cats[cat["id"]] = cat
        if "annotations" in self.dataset and "categories" in self.dataset:
            for ann in self.dataset["annotations"]:
                catToImgs[ann["category_id"]].append(ann["image_id"])
        self.anns, self.imgToAnns, self.catToImgs, self.imgs, self.cats = anns, imgToAnns, catToImgs, imgs, cats

    def getAnnIds(self, imgIds=[], catIds=[]):
        imgIds = imgIds if isinstance(imgIds, (list, tuple)) else [imgIds]
        catIds = catIds if isinstance(catIds, (list, tuple)) else [catIds]
        if len(imgIds) == 0:
            anns = self.dataset.get("annotations", [])
        else:
            anns = [a for i in imgIds if i in self.imgToAnns for a in self.imgToAnns[i]]
        if len(catIds):
            anns = [a for a in anns if a["category_id"] in catIds]
        return [a["id"] for a in anns]

    def getCatIds(self, catNms=[]):
        cats = self.dataset["categories"]
        if len(catNms):
            cats = [c for c in cats if c["name"] in catNms]
        return [c["id"] for c in cats]

    def getImgIds(self):
        return list(self.imgs.keys())

    def loadAnns(self, ids=[]):
        return [self.anns[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.anns[ids]]

    def loadCats(self, ids=[]):
        return [self.cats[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.cats[ids]]

    def get_ann_ids(self, img_ids=[], cat_ids=[]):
        return self.getAnnIds(img_ids, cat_ids)

    def get_cat_ids(self, cat_names=[]):
        return self.getCatIds(list(cat_names))

    def get_img_ids(self):
        return self.getImgIds()

    load_anns, load_cats = loadAnns, loadCats

    def loadRes(self, anns):
        res = COCO()
        res.dataset["images"] = [img for img in self.dataset["images"]]
        assert isinstance(anns, list), "results in not an array of objects"
        ids = [a["image_id"] for a in anns]
        assert set(ids) == (set(ids) & set(self.getImgIds())), "Results do not correspond to current coco set"
        if "bbox" in anns[0] and not anns[0]["bbox"] == []:      # IndexError on an empty list, as upstream
            res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
            for i, ann in enumerate(anns):
                bb = ann["bbox"]
                ann["area"] = bb[2] * bb[3]
                ann["id"] = i + 1
                ann["iscrowd"] = 0
        elif "segmentation" in anns[0]:
            res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
            for i, ann in enumerate(anns):
                ann["area"] = int(decode_mask(ann["segmentation"]).sum())
                ann["id"] = i + 1
                ann["iscrowd"] = 0
        res.dataset["annotations"] = anns
        res.createIndex()
        return res


# ---------------------------------------------------------------------------------------------------------------- COCOeval
class Params:
    def __init__(self, iouType="segm"):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [list(r) for r in AREA_RNG]
        self.areaRngLbl = list(AREA_LBL)
        self.useCats = 1
        self.iouType = iouType


def match_sequential(ious, thrs, gt_ig, crowd):
    """evaluateImg's loop, literally.  ious (D, G) with the gts in sorted order, gt_ig / crowd (G).  -> m (T, D): the matched gt position or -1"""
    T, (D, G) = len(thrs), ious.shape
    gtm, out = np.zeros((T, G), bool), -np.ones((T, D), np.int64)
    for tind, t in enumerate(thrs):
        for dind in range(D):
            iou, m = min([t, 1 - 1e-10]), -1
            for gind in range(G):
                if gtm[tind, gind] and not crowd[gind]:
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break
                if ious[dind, gind] < iou:
                    continue
                iou, m = ious[dind, gind], gind
            if m == -1:
                continue
            out[tind, dind], gtm[tind, m] = m, True
    return out


def match_two_sections(ious, thrs, gt_ig, crowd):
    """the same result in the form the kernel uses: the largest IoU >= min(t, 1 - 1e-10) among the available non-ignored gts, the highest position
    among equal IoUs; if there is none, the same among the ignored ones"""
    T, (D, G) = len(thrs), ious.shape
    gtm, out = np.zeros((T, G), bool), -np.ones((T, D), np.int64)
    for tind, t in enumerate(thrs):
        thr = min([t, 1 - 1e-10])
        for dind in range(D):
            for section in (0, 1):
                cand = [g for g in range(G) if gt_ig[g] == section and (not gtm[tind, g] or crowd[g]) and ious[dind, g] >= thr]
                if cand:
                    top = max(ious[dind, g] for g in cand)
                    m = max(g for g in cand if ious[dind, g] == top)
                    out[tind, dind], gtm[tind, m] = m, True
                    break
    return out


def accumulate_segment(dtm, dt_ig, scores, npig, rec_thrs):
    """COCOeval.accumulate's body for one (k, a, m): dtm / dt_ig (T, n) bool in concatenation order, scores (n) -> precision (T, R), scores (T, R),
    recall (T); npig > 0"""
    T, R = dtm.shape[0], len(rec_thrs)
    inds = np.argsort(-scores, kind="mergesort")
    sorted_scores = scores[inds]
    dtm, dt_ig = dtm[:, inds], dt_ig[:, inds]
    tps, fps = np.logical_and(dtm, np.logical_not(dt_ig)), np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
    tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(dtype=float), np.cumsum(fps, axis=1).astype(dtype=float)
    precision, out_scores, recall = np.zeros((T, R)), np.zeros((T, R)), np.zeros(T)
    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
        tp, fp = np.array(tp), np.array(fp)
        nd = len(tp)
        rc = tp / npig
        pr = tp / (fp + tp + np.spacing(1))
        q, ss = np.zeros((R,)), np.zeros((R,))
        recall[t] = rc[-1] if nd else 0
        pr, q = pr.tolist(), q.tolist()
        for i in range(nd - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        at = np.searchsorted(rc, rec_thrs, side="left")
        try:
            for ri, pi in enumerate(at):
                q[ri] = pr[pi]
                ss[ri] = sorted_scores[pi]
        except IndexError:
            pass
        precision[t], out_scores[t] = np.array(q), np.array(ss)
    return precision, out_scores, recall


class COCOeval:
    def __init__(self, cocoGt=None, cocoDt=None, iouType="segm"):
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.evalImgs, self.eval = defaultdict(list), {}
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        self.params = Params(iouType=iouType)
        self._paramsEval, self.stats, self.ious = {}, [], {}
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    def _prepare(self):
        p = self.params
        if p.useCats:
            gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
            dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        else:
            gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds))
            dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds))
        if p.iouType == "segm":
            for ann in gts + dts:
                ann["_mask"] = decode_mask(ann["segmentation"])
        for gt in gts:
            gt["ignore"] = gt["ignore"] if "ignore" in gt else 0
            gt["ignore"] = "iscrowd" in gt and gt["iscrowd"]
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for gt in gts:
            self._gts[gt["image_id"], gt["category_id"]].append(gt)
        for dt in dts:
            self._dts[dt["image_id"], dt["category_id"]].append(dt)
        self.evalImgs, self.eval = defaultdict(list), {}

    def _cell(self, imgId, catId):
        p = self.params
        if p.useCats:
            return self._gts[imgId, catId], self._dts[imgId, catId]
        return [_ for cId in p.catIds for _ in self._gts[imgId, cId]], [_ for cId in p.catIds for _ in self._dts[imgId, cId]]

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        if p.useCats:
            p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self.params = p
        self._prepare()
        catIds = p.catIds if p.useCats else [-1]
        self.ious = {(imgId, catId): self.computeIoU(imgId, catId) for imgId in p.imgIds for catId in catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet) for catId in catIds for areaRng in p.areaRng for imgId in p.imgIds]
        self._paramsEval = copy.deepcopy(self.params)

    def computeIoU(self, imgId, catId):
        p = self.params
        gt, dt = self._cell(imgId, catId)
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds]
        if len(dt) > p.maxDets[-1]:
            dt = dt[0:p.maxDets[-1]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        if len(dt) == 0 or len(gt) == 0:
            return []
        if p.iouType == "segm":
            return mask_iou(np.stack([d["_mask"] for d in dt]), np.stack([g["_mask"] for g in gt]), iscrowd)[0]
        return bbox_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], iscrowd)

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt, dt = self._cell(imgId, catId)
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if g["ignore"] or (g["area"] < aRng[0] or g["area"] > aRng[1]) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T, G, D = len(p.iouThrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gtIg = np.array([g["_ignore"] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            m = match_sequential(ious, p.iouThrs, gtIg, iscrowd)
            for tind in range(T):
                for dind in range(D):
                    if m[tind, dind] >= 0:
                        dtIg[tind, dind] = gtIg[m[tind, dind]]
                        dtm[tind, dind] = gt[m[tind, dind]]["id"]
                        gtm[tind, m[tind, dind]] = dt[dind]["id"]
        a = np.array([d["area"] < aRng[0] or d["area"] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return dict(image_id=imgId, category_id=catId, aRng=aRng, maxDet=maxDet, dtIds=[d["id"] for d in dt], gtIds=[g["id"] for g in gt], dtMatches=dtm,
                    gtMatches=gtm, dtScores=[d["score"] for d in dt], gtIgnore=gtIg, dtIgnore=dtIg)

    def accumulate(self):
        p = self._paramsEval
        catIds = p.catIds if p.useCats else [-1]
        T, R, K, A, M, I = len(p.iouThrs), len(p.recThrs), len(catIds), len(p.areaRng), len(p.maxDets), len(p.imgIds)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        for k in range(K):
            for a in range(A):
                for m, maxDet in enumerate(p.maxDets):
                    E = [self.evalImgs[k * A * I + a * I + i] for i in range(I)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                    dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)
                    dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)
                    gtIg = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    pr, ss, rc = accumulate_segment(dtm != 0, dtIg != 0, np.asarray(dtScores, np.float64), npig, p.recThrs)
                    precision[:, :, k, a, m], scores[:, :, k, a, m], recall[:, k, a, m] = pr, ss, rc
        self.eval = dict(params=p, counts=[T, R, K, A, M], precision=precision, recall=recall, scores=scores)

    def summarize(self):
        p = self.params

        def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            s = self.eval["precision"] if ap == 1 else self.eval["recall"]
            if iouThr is not None:
                s = s[np.where(iouThr == p.iouThrs)[0]]
            s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        stats = np.zeros((12,))
        stats[0] = _summarize(1, maxDets=p.maxDets[2])
        stats[1] = _summarize(1, iouThr=.5, maxDets=p.maxDets[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=p.maxDets[2])
        stats[3] = _summarize(1, areaRng="small", maxDets=p.maxDets[2])
        stats[4] = _summarize(1, areaRng="medium", maxDets=p.maxDets[2])
        stats[5] = _summarize(1, areaRng="large", maxDets=p.maxDets[2])
        stats[6] = _summarize(0, maxDets=p.maxDets[0])
        stats[7] = _summarize(0, maxDets=p.maxDets[1])
        stats[8] = _summarize(0, maxDets=p.maxDets[2])
        stats[9] = _summarize(0, areaRng="small", maxDets=p.maxDets[2])
        stats[10] = _summarize(0, areaRng="medium", maxDets=p.maxDets[2])
        stats[11] = _summarize(0, areaRng="large", maxDets=p.maxDets[2])
        self.stats = stats


# ---------------------------------------------------------------------------------------------------------------- the reference's conversions
def xyxy2xywh(bbox):
    """metric.py:185-203: tolist() of the float32 corners, the differences in Python floats"""
    b = np.asarray(bbox).tolist()
    return [b[0], b[1], b[2] - b[0], b[3] - b[1]]


def to_coco(images, num_classes, kind):
    """images: dicts with img_id, height, width, bboxes (D, 4) f32, scores, labels, masks (D, H, W) bool or None, gt_bboxes, gt_labels, gt_ignore,
    gt_masks.  -> (gt dataset dict as gt_to_coco_json builds it, prediction list as results2json + the 'bbox' pop of compute_metrics leave it)"""
    cats = [dict(id=k, name="c%d" % k) for k in range(num_classes)]
    infos, anns, preds = [], [], []
    for im in images:
        infos.append(dict(id=im["img_id"], width=im["width"], height=im["height"], file_name=""))
        gm = encode_masks(im["gt_masks"]) if im.get("gt_masks") is not None else None
        for j in range(len(im["gt_labels"])):
            cb = xyxy2xywh(im["gt_bboxes"][j])
            ann = dict(id=len(anns) + 1, image_id=im["img_id"], bbox=cb, iscrowd=int(im["gt_ignore"][j]), category_id=int(im["gt_labels"][j]), area=cb[2] * cb[3])
            if gm is not None:
                ann["segmentation"] = gm[j]
            anns.append(ann)
        dm = encode_masks(im["masks"]) if kind == "segm" else None
        for j in range(len(im["labels"])):
            d = dict(image_id=im["img_id"], score=float(im["scores"][j]), category_id=int(im["labels"][j]))
            if kind == "segm":
                d["segmentation"] = dm[j]
            else:
                d["bbox"] = xyxy2xywh(im["bboxes"][j])
            preds.append(d)
    gt = dict(images=infos, categories=cats, licenses=None)
    if anns:
        gt["annotations"] = anns
    return gt, preds


def evaluate(images, kind, num_classes, iou_thrs=None, max_dets=(100, 300, 1000)):
    """kind 'bbox' | 'segm' | 'proposal' -> the COCOeval after evaluate / accumulate / summarize (None when there is no detection at all)"""
    gt, preds = to_coco(images, num_classes, "segm" if kind == "segm" else "bbox")
    api = COCO(gt)
    if not preds:
        return None
    E = COCOeval(api, api.loadRes(preds), "segm" if kind == "segm" else "bbox")
    E.params.catIds, E.params.imgIds, E.params.maxDets = api.getCatIds(), api.getImgIds(), list(max_dets)
    if iou_thrs is not None:
        E.params.iouThrs = np.asarray(iou_thrs, np.float64)
    if kind == "proposal":
        E.params.useCats = 0
    E.evaluate()
    E.accumulate()
    E.summarize()
    return E


def list_flags(E):
    """the evaluation in the kernels' LIST ORDER (cell by cell: images in p.imgIds order x categories, inside a cell by score rank, EVERY detection of
    the cell, also those past maxDets[-1], which carry zeros) -> matched, ignored (A, T, D) uint8, rank (D) int32, score (D) float64, label (D) int64
    (0 without useCats), npig (K, A) int64"""
    p = E._paramsEval
    catIds = p.catIds if p.useCats else [-1]
    A, T, I, K = len(p.areaRng), len(p.iouThrs), len(p.imgIds), len(catIds)
    matched, ignored, rank, score, label = [[] for _ in range(A)], [[] for _ in range(A)], [], [], []
    npig = np.zeros((K, A), np.int64)
    for i, imgId in enumerate(p.imgIds):
        for k, catId in enumerate(catIds):
            dt = E._cell(imgId, catId)[1]
            s = np.array([d["score"] for d in dt], np.float64)
            s = s[np.argsort(-s, kind="mergesort")]
            n = len(dt)
            rank += list(range(n))
            score += s.tolist()
            label += [k] * n
            for a in range(A):
                e = E.evalImgs[k * A * I + a * I + i]
                m, g = np.zeros((T, n), np.uint8), np.zeros((T, n), np.uint8)
                if e is not None:
                    kept = e["dtMatches"].shape[1]
                    m[:, :kept], g[:, :kept] = e["dtMatches"] != 0, e["dtIgnore"] != 0
                    npig[k, a] += np.count_nonzero(e["gtIgnore"] == 0)
                matched[a].append(m), ignored[a].append(g)
    cat = lambda rows: np.stack([np.concatenate(r, axis=1) if r else np.zeros((T, 0), np.uint8) for r in rows])      # noqa: E731
    return cat(matched), cat(ignored), np.array(rank, np.int32), np.array(score, np.float64), np.array(label, np.int64), npig


METRIC_NAMES = {"mAP": 0, "mAP_50": 1, "mAP_75": 2, "mAP_s": 3, "mAP_m": 4, "mAP_l": 5, "AR@100": 6, "AR@300": 7, "AR@1000": 8, "AR_s@1000": 9,
                "AR_m@1000": 10, "AR_l@1000": 11}


def metrics_dict(stats, precision, metric, class_names, classwise=False, metric_items=None):
    """the result dict as metric.py:493-580 fills it from coco_eval.stats / eval['precision']"""
    out = {}
    if metric == "proposal":
        for item in metric_items or ["AR@100", "AR@300", "AR@1000", "AR_s@1000", "AR_m@1000", "AR_l@1000"]:
            out[item] = float(f"{stats[METRIC_NAMES[item]]:.3f}")
        return out
    if classwise:
        for idx, name in enumerate(class_names):
            pr = precision[:, :, idx, 0, -1]
            pr = pr[pr > -1]
            out[f"{name}_precision"] = round(np.mean(pr) if pr.size else float("nan"), 3)
    for item in metric_items or ["mAP", "mAP_50", "mAP_75", "mAP_s", "mAP_m", "mAP_l"]:
        out[f"{metric}_{item}"] = float(f"{round(stats[METRIC_NAMES[item]], 3)}")
    return out
