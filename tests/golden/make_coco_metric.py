"""Generate f27_coco_metric.npz: the reference's own COCO metric (Multi-Task_Pretrain/instance_segmentation/metric.py: MTP_IS_Metric.process /
compute_metrics / gt_to_coco_json / results2json / xyxy2xywh) run on the set 'fixture' of tests/coco_eval_cases.py.

Runs in the development container only (the reference is not on the GPU machine).  metric.py is imported by path; what it imports from mmengine /
mmdet / terminaltables is not installed, so each of those is restated below and labelled STUB (the method of make_dota_metric.py).  pycocotools is
not installed either: mmdet.datasets.api_wrappers.COCO / COCOeval are served by the numpy restatement tests/coco_eval_ref.py, and
encode_mask_results by its lossless stand-in for the run-length encoding.  So the fixture pins the reference's OWN code -- process, gt_to_coco_json,
results2json, the json round trip through files, the 'bbox' pop for 'segm', the parameters it sets on COCOeval, the key names and the rounding --
and NOT the arithmetic of COCOeval, which rests on the restatement.

Recorded: the inputs; the parameters the reference set on each COCOeval; per metric ('bbox', 'segm', 'proposal') the restatement's arrays as the
reference drove it (precision, recall, scores, stats, and the flags in list order); the compute_metrics dict of metric=['bbox', 'segm', 'proposal']
with classwise=True.  Fixed time stamps: the archive regenerates bit for bit.

    python tests/golden/make_coco_metric.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import coco_eval_cases as C  # noqa: E402
import coco_eval_ref as R  # noqa: E402
from make_dota_metric import write_npz  # noqa: E402

REF = "/root/reference/Multi-Task_Pretrain/instance_segmentation/metric.py"
METRICS = ("bbox", "segm", "proposal")
EVALS = []      # every COCOeval the reference built, in order


# ---------------------------------------------------------------------------------------------------------------- STUBS
class BaseMetric:
    """STUB of mmengine.evaluator.BaseMetric: the result list and the attributes the metric reads"""

    def __init__(self, collect_device="cpu", prefix=None):
        self.results, self.prefix, self.dataset_meta = [], prefix, None


class MMLogger:
    """STUB of mmengine.logging.MMLogger"""

    @staticmethod
    def get_current_instance():
        return MMLogger()

    def info(self, *a, **k):
        pass

    error = info


def dump(obj, path):
    """STUB of mmengine.fileio.dump (json by extension)"""
    with open(path, "w") as f:
        json.dump(obj, f)


def load(path):
    """STUB of mmengine.fileio.load (json by extension)"""
    with open(path) as f:
        return json.load(f)


def _unused(*a, **k):
    """STUB of a symbol the reference imports and this run never calls (get_local_path: ann_file; eval_recalls: 'proposal_fast')"""
    raise NotImplementedError


class AsciiTable:
    """STUB of terminaltables.AsciiTable"""

    def __init__(self, data):
        self.table = "\n".join(" | ".join(str(c) for c in row) for row in data)


class _Registry:
    """STUB of mmdet.registry.METRICS"""

    def register_module(self, *a, **k):
        return lambda cls: cls


class SpyCOCOeval(R.COCOeval):
    """the restatement's COCOeval, remembered so that what the reference set on it and what it computed can be recorded"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        EVALS.append(self)


def encode_mask_results(masks):
    """STUB of mmdet.structures.mask.encode_mask_results: the restatement's lossless, json-able encoding"""
    return R.encode_masks(masks)


def _install_stubs():
    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmengine"), mod("mmengine.evaluator", BaseMetric=BaseMetric), mod("mmengine.fileio", dump=dump, load=load, get_local_path=_unused)
    mod("mmengine.logging", MMLogger=MMLogger)
    mod("terminaltables", AsciiTable=AsciiTable)
    mod("mmdet"), mod("mmdet.datasets"), mod("mmdet.datasets.api_wrappers", COCO=R.COCO, COCOeval=SpyCOCOeval)
    mod("mmdet.registry", METRICS=_Registry()), mod("mmdet.structures"), mod("mmdet.structures.mask", encode_mask_results=encode_mask_results)
    mod("mmdet.evaluation"), mod("mmdet.evaluation.functional", eval_recalls=_unused)


def _load():
    _install_stubs()
    spec = importlib.util.spec_from_file_location("ref_is_metric", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Sample(dict):
    """a data sample as the reference's process reads it: attributes, and `'instances' in sample`"""
    __getattr__ = dict.__getitem__


def samples(images):
    """the images of coco_eval_cases as data samples: predictions as tensors, the ground truth as the dataset's `instances` (Python floats, encoded
    masks)"""
    out = []
    for im in images:
        t = torch.from_numpy
        pred = dict(bboxes=t(im["bboxes"].copy()), scores=t(im["scores"].copy()), labels=t(im["labels"].copy()), masks=t(im["masks"].copy()))
        enc = R.encode_masks(im["gt_masks"])
        inst = [dict(bbox_label=int(im["gt_labels"][j]), bbox=im["gt_bboxes"][j].tolist(), ignore_flag=int(im["gt_ignore"][j]), mask=enc[j])
                for j in range(len(im["gt_labels"]))]
        out.append(Sample(img_id=im["img_id"], ori_shape=(im["height"], im["width"]), pred_instances=pred, instances=inst))
    return out


def inputs(images):
    """the set as flat arrays (masks as bit-packed rows)"""
    cat = lambda k, empty: np.concatenate([im[k] for im in images]) if images else empty      # noqa: E731
    return {"in.det_count": np.array([len(im["labels"]) for im in images]), "in.gt_count": np.array([len(im["gt_labels"]) for im in images]),
            "in.img_id": np.array([im["img_id"] for im in images]), "in.size": np.array([[im["height"], im["width"]] for im in images]),
            "in.bboxes": cat("bboxes", None), "in.scores": cat("scores", None), "in.labels": cat("labels", None),
            "in.masks": np.packbits(cat("masks", None).reshape(-1, C.H * C.W), axis=1), "in.gt_bboxes": cat("gt_bboxes", None),
            "in.gt_labels": cat("gt_labels", None), "in.gt_ignore": cat("gt_ignore", None),
            "in.gt_masks": np.packbits(cat("gt_masks", None).reshape(-1, C.H * C.W), axis=1)}


def build():
    m = _load()
    images, K, max_dets = C.case("fixture")
    names = tuple("c%d" % k for k in range(K))
    out = inputs(images)
    out["seed"] = np.array(C.SEEDS["fixture"])
    del EVALS[:]
    metric = m.MTP_IS_Metric(metric=list(METRICS), classwise=True, proposal_nums=max_dets)
    metric.dataset_meta = dict(classes=names)
    metric.process(None, samples(images))
    got = metric.compute_metrics(metric.results)
    assert len(EVALS) == len(METRICS)
    out["metrics.keys"] = np.array(list(got.keys()))
    out["metrics.values"] = np.array([float(v) for v in got.values()])
    for kind, E in zip(METRICS, EVALS):
        p = E._paramsEval
        out[kind + ".iouType"], out[kind + ".useCats"] = np.array(p.iouType), np.array(p.useCats)
        out[kind + ".imgIds"], out[kind + ".catIds"] = np.array(p.imgIds, np.int64), np.array(p.catIds, np.int64)
        out[kind + ".maxDets"], out[kind + ".iouThrs"] = np.array(p.maxDets, np.int64), np.array(p.iouThrs, np.float64)
        out[kind + ".dt_area"] = np.array([a["area"] for a in E.cocoDt.dataset["annotations"]], np.float64)
        out[kind + ".gt_area"] = np.array([a["area"] for a in E.cocoGt.dataset["annotations"]], np.float64)
        out[kind + ".gt_bbox"] = np.array([a["bbox"] for a in E.cocoGt.dataset["annotations"]], np.float64)
        if kind != "segm":
            out[kind + ".dt_bbox"] = np.array([a["bbox"] for a in E.cocoDt.dataset["annotations"]], np.float64)
        for k in ("precision", "recall", "scores"):
            out["%s.%s" % (kind, k)] = E.eval[k]
        out[kind + ".stats"] = np.asarray(E.stats, np.float64)
        for k, v in zip(("matched", "ignored", "rank", "score", "label", "npig"), R.list_flags(E)):
            out["%s.list.%s" % (kind, k)] = v
    return out


def main():
    path = os.path.join(HERE, "f27_coco_metric.npz")
    write_npz(path, build())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
