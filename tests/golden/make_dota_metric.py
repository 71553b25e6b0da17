"""Generate f24_dota_metric.npz: the reference's own DOTA metric (Multi-Task_Pretrain/rotated_detection/metric.py: MTP_RD_Metric.process /
compute_metrics / merge_results, eval_rbbox_map, get_cls_results, tpfp_default) run on the set 'fixture' of tests/det_eval_cases.py.

Runs in the development container only (the reference is not on the GPU machine).  metric.py is imported by path; what it imports from mmcv / mmengine
/ mmrotate / mmdet / terminaltables is not installed, so each of those is restated below from the published algorithm and labelled STUB (the method of
make_oriented_rpn.py; this file carries its own stubs).  box_iou_rotated / nms_rotated call tests/box_ref.py in float64 on the float32 inputs and
round the IoU to float32 (mmcv returns float32); average_precision is the restatement of tests/det_eval_ref.py.  The control flow is the reference's
own: process, compute_metrics, results2json, eval_rbbox_map, get_cls_results, tpfp_default, print_map_summary, merge_results.

Recorded: the inputs; for iou_thr 0.5 and 0.75 and both eval modes the per-class tp / fp (image order, as tpfp_default returned them), num_gts,
num_dets, recall, precision, ap and the mean; the compute_metrics dict of iou_thrs=[0.5, 0.75] in both modes; and the Task1_<class>.txt files of
merge_patches=True over the same detections under patch ids.  Fixed time stamps: the archive regenerates bit for bit.

    python tests/golden/make_dota_metric.py
"""
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import box_ref as BR  # noqa: E402
import det_eval_cases as C  # noqa: E402
import det_eval_ref as R  # noqa: E402

REF = "/root/reference/Multi-Task_Pretrain/rotated_detection/metric.py"
CLASSES = ("plane", "ship", "storage-tank", "harbor")
THRS = (0.5, 0.75)
# the patch ids of the merge run: the six images as patches of two originals (name__size__x___y)
PATCH_IDS = ("P0007__1024__0___0", "P0007__1024__824___0", "P0007__1024__0___824", "P0003__1024__0___0", "P0003__1024__824___824", "P0003__1024__1648___0")
MERGE_IOU_THR = 0.1


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


def print_log(*a, **k):
    """STUB of mmengine.logging.print_log"""


def dump(obj, path):
    """STUB of mmengine.fileio.dump (json by extension)"""
    with open(path, "w") as f:
        json.dump(obj, f)


class AsciiTable:
    """STUB of terminaltables.AsciiTable"""

    def __init__(self, data):
        self.table = "\n".join(" | ".join(str(c) for c in row) for row in data)


class _Registry:
    """STUB of mmrotate.registry.METRICS"""

    def register_module(self, *a, **k):
        return lambda cls: cls


def box_iou_rotated(b1, b2, *a, **k):
    """STUB of mmcv.ops.box_iou_rotated: box_ref in float64, rounded to float32.  The reference passes the (m, 6) detections, score column included:
    the first five columns are the box."""
    return torch.from_numpy(BR.box_iou_rotated(b1.numpy()[:, :5], b2.numpy()[:, :5]).astype(np.float32))


def nms_rotated(dets, scores, iou_threshold, labels=None):
    """STUB of mmcv.ops.nms_rotated: greedy, descending score (stable) -> (dets with scores (k, 6), kept indices)"""
    keep = torch.from_numpy(BR.nms(dets.numpy(), scores.numpy(), iou_threshold, rotated=True))
    return torch.cat([dets[keep], scores[keep, None]], 1), keep


def _unused(*a, **k):
    """STUB of a symbol the reference imports and this run never calls"""
    raise NotImplementedError


def rbox2qbox(boxes):
    """STUB of mmrotate.structures.bbox.rbox2qbox: the corners centre + u + v, centre + u - v, centre - u - v, centre - u + v with u = w / 2 (cos, sin)
    and v = h / 2 (-sin, cos)"""
    ctr, w, h, theta = torch.split(boxes, (2, 1, 1, 1), dim=-1)
    cos_value, sin_value = torch.cos(theta), torch.sin(theta)
    vec1 = torch.cat([w / 2 * cos_value, w / 2 * sin_value], dim=-1)
    vec2 = torch.cat([-h / 2 * sin_value, h / 2 * cos_value], dim=-1)
    return torch.cat([ctr + vec1 + vec2, ctr + vec1 - vec2, ctr - vec1 - vec2, ctr - vec1 + vec2], dim=-1)


def _install_stubs():
    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmcv"), mod("mmcv.ops", nms_quadri=_unused, nms_rotated=nms_rotated, box_iou_quadri=_unused, box_iou_rotated=box_iou_rotated)
    mod("mmengine"), mod("mmengine.evaluator", BaseMetric=BaseMetric), mod("mmengine.fileio", dump=dump)
    mod("mmengine.logging", MMLogger=MMLogger, print_log=print_log)
    mod("mmrotate"), mod("mmrotate.evaluation", eval_rbbox_map=_unused), mod("mmrotate.registry", METRICS=_Registry())
    mod("mmrotate.structures"), mod("mmrotate.structures.bbox", rbox2qbox=rbox2qbox)
    mod("mmdet"), mod("mmdet.evaluation"), mod("mmdet.evaluation.functional", average_precision=R.average_precision)
    mod("terminaltables", AsciiTable=AsciiTable)


def _load():
    _install_stubs()
    spec = importlib.util.spec_from_file_location("ref_rd_metric", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class Sample:
    """a data sample as the reference's process reads it"""

    def __init__(self, img_id, pred, gt, ignored):
        self.img_id, self.r_pred_instances, self.r_gt_instances, self.r_ignored_instances = img_id, pred, gt, ignored


def samples(ids=None):
    """the set 'fixture' as data samples: float32 tensors, the detections of an image in table order (class by class)"""
    det_results, annotations = C.case("fixture")
    out = []
    for i, (res, ann) in enumerate(zip(det_results, annotations)):
        d = np.vstack(res).astype(np.float32)
        labels = np.concatenate([np.full(len(r), k, np.int64) for k, r in enumerate(res)])
        t = torch.from_numpy
        out.append(Sample(i if ids is None else ids[i], dict(bboxes=t(d[:, :5].copy()), scores=t(d[:, 5].copy()), labels=t(labels)),
                          dict(bboxes=t(ann["bboxes"].astype(np.float32)), labels=t(ann["labels"])),
                          dict(bboxes=t(ann["bboxes_ignore"].astype(np.float32)), labels=t(ann["labels_ignore"]))))
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and a sorted order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def build():
    m = _load()
    out = {}
    tb = R.tables(*C.case("fixture"))
    for k, v in tb.items():
        out["in." + k] = v
    out["seed"] = np.array(C.SEEDS["fixture"])
    for mode in ("11points", "area"):
        metric = m.MTP_RD_Metric(iou_thrs=list(THRS), eval_mode=mode)
        metric.dataset_meta = dict(classes=CLASSES)
        metric.process(None, samples())
        gts, preds = zip(*metric.results)
        dets = [p["pred_bbox_scores"] for p in preds]
        for thr in THRS:
            calls, inner = [], m.tpfp_default

            def spy(*a, **k):
                calls.append(inner(*a, **k))
                return calls[-1]
            m.tpfp_default = spy
            mean_ap, res = m.eval_rbbox_map(dets, gts, iou_thr=thr, use_07_metric=mode == "11points", dataset=CLASSES, logger="silent")
            m.tpfp_default = inner
            p = "%s.thr%02d." % (mode, int(thr * 100))
            out[p + "mean_ap"] = np.array(mean_ap)
            n = len(dets)
            for c, r in enumerate(res):
                q = "%scls%d." % (p, c)
                assert r["recall"].dtype == np.float64 and r["precision"].dtype == np.float32 and np.asarray(r["ap"]).dtype == np.float32
                out[q + "tp"] = np.hstack([t[0] for t in calls[c * n:(c + 1) * n]])[0].astype(np.uint8)
                out[q + "fp"] = np.hstack([t[1] for t in calls[c * n:(c + 1) * n]])[0].astype(np.uint8)
                out[q + "num_gts"], out[q + "num_dets"] = np.array(r["num_gts"]), np.array(r["num_dets"])
                out[q + "recall"], out[q + "precision"], out[q + "ap"] = r["recall"], r["precision"], np.array(r["ap"])
        got = metric.compute_metrics(metric.results)
        out[mode + ".metrics.keys"] = np.array(list(got.keys()))
        out[mode + ".metrics.values"] = np.array([float(v) for v in got.values()])
    with tempfile.TemporaryDirectory() as tmp:
        metric = m.MTP_RD_Metric(merge_patches=True, iou_thr=MERGE_IOU_THR, outfile_prefix=os.path.join(tmp, "Task1"))
        metric.dataset_meta = dict(classes=CLASSES)
        metric.process(None, samples(PATCH_IDS))
        assert metric.compute_metrics(metric.results) == {}
        for c in CLASSES:
            out["merge.Task1_%s.txt" % c] = np.frombuffer(open(os.path.join(tmp, "Task1", "Task1_%s.txt" % c), "rb").read(), np.uint8)
        assert sorted(zipfile.ZipFile(os.path.join(tmp, "Task1", "Task1.zip")).namelist()) == sorted("Task1_%s.txt" % c for c in CLASSES)
    return out


def main():
    path = os.path.join(HERE, "f24_dota_metric.npz")
    write_npz(path, build())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
