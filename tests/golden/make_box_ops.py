"""Generate f21_box_ops.npz: the reference's own MTP_RD_MaxIoUAssigner (Multi-Task_Pretrain/rotated_detection/max_iou_assigner.py) run in float64.

Runs in the development container only (the reference is not on the GPU machine).  max_iou_assigner.py is imported by path; what it imports from
mmengine / mmdet / mmrotate is not installed, so each of those is restated below from the published algorithm and labelled STUB: InstanceData (a bag of
attributes), the TASK_UTILS registry, AssignResult, BaseAssigner, HorizontalBoxes / RotatedBoxes (.tensor, convert_to('hbox')), get_box_tensor,
bbox_overlaps, rbbox_overlaps and the calculators BboxOverlaps2D / RBboxOverlaps2D.  The stubbed overlaps call tests/box_ref.py in float64; the
assignment itself -- assign(), assign_wrt_overlaps(), and the rotated -> box calculator MTP_RD_RBbox2HBboxOverlaps2D -- is the reference's code.
Recorded: one input set per calculator kind (12 gts, 300 priors, rounded to float32 and stored so; the first seeds that meet box_cases.assign_condition)
and the results (gt_inds, max_overlaps, labels) under the four configurations of oriented_rcnn.py:78-108 / mask_rcnn.py:72-99, one with
gt_max_assign_all=False and one with a neg_iou_thr pair.  The archive is written with fixed time stamps: it regenerates bit for bit.

    python tests/golden/make_box_ops.py
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import box_cases as C  # noqa: E402
import box_ref as R  # noqa: E402

REF = "/root/reference/Multi-Task_Pretrain/rotated_detection/max_iou_assigner.py"
K, N = 12, 300
# (configuration of box_cases.ASSIGN_CFGS, calculator kind)
RUNS = (("rpn", "rbox2hbox"), ("rcnn_off", "rotated"), ("rpn", "box"), ("rcnn_on", "box"), ("first_only", "rbox2hbox"), ("neg_pair", "rotated"))
CALCULATOR = {"box": "BboxOverlaps2D", "rbox2hbox": "MTP_RD_RBbox2HBboxOverlaps2D", "rotated": "RBboxOverlaps2D"}


# ---------------------------------------------------------------------------------------------------------------- STUBS
class InstanceData:
    """STUB of mmengine.structures.InstanceData: a bag of attributes"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Registry:
    """STUB of mmengine's Registry: register_module() as a decorator, build(cfg)"""

    def __init__(self):
        self.modules = {}

    def register_module(self, *a, **k):
        def deco(cls):
            self.modules[cls.__name__] = cls
            return cls
        return deco

    def build(self, cfg):
        cfg = dict(cfg)
        return self.modules[cfg.pop("type")](**cfg)


TASK_UTILS = _Registry()


class AssignResult:
    """STUB of mmdet's AssignResult"""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class BaseAssigner:
    """STUB of mmdet's BaseAssigner (an abstract base)"""


class _Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


class HorizontalBoxes(_Boxes):
    """STUB of mmdet.structures.bbox.HorizontalBoxes"""


class QuadriBoxes(_Boxes):
    """STUB of mmrotate.structures.bbox.QuadriBoxes (imported by the reference, unused)"""


class RotatedBoxes(_Boxes):
    """STUB of mmrotate.structures.bbox.RotatedBoxes: convert_to('hbox') is the circumscribed box"""

    def convert_to(self, kind):
        assert kind == "hbox"
        return HorizontalBoxes(torch.from_numpy(R.rbox2hbox(self.tensor.numpy())))


def get_box_tensor(b):
    """STUB of mmdet.structures.bbox.get_box_tensor"""
    return b.tensor if isinstance(b, _Boxes) else b


def bbox_overlaps(b1, b2, mode="iou", is_aligned=False, eps=1e-6):
    """STUB of mmdet.structures.bbox.bbox_overlaps"""
    return torch.from_numpy(R.bbox_overlaps(b1.numpy(), b2.numpy(), mode, is_aligned, eps))


def rbbox_overlaps(b1, b2, mode="iou", is_aligned=False):
    """STUB of mmrotate.structures.bbox.rbbox_overlaps (mmcv's box_iou_rotated)"""
    return torch.from_numpy(R.box_iou_rotated(b1.numpy(), b2.numpy(), mode, is_aligned))


def fake_rbbox_overlaps(*a, **k):
    """STUB of mmrotate.structures.bbox.fake_rbbox_overlaps (imported by the reference, unused)"""
    raise NotImplementedError


def cast_tensor_type(x, scale=1., dtype=None):
    """STUB of mmrotate's cast_tensor_type (the fp16 path, not taken)"""
    raise NotImplementedError


@TASK_UTILS.register_module()
class BboxOverlaps2D:
    """STUB of mmdet's BboxOverlaps2D"""

    def __init__(self, scale=1., dtype=None):
        assert dtype is None

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        return bbox_overlaps(get_box_tensor(bboxes1), get_box_tensor(bboxes2), mode, is_aligned)


@TASK_UTILS.register_module()
class RBboxOverlaps2D:
    """STUB of mmrotate's RBboxOverlaps2D"""

    def __init__(self, scale=1., dtype=None):
        assert dtype is None

    def __call__(self, bboxes1, bboxes2, mode="iou", is_aligned=False):
        return rbbox_overlaps(get_box_tensor(bboxes1), get_box_tensor(bboxes2), mode, is_aligned)


def _install_stubs():
    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmengine"), mod("mmengine.structures", InstanceData=InstanceData)
    mod("mmdet"), mod("mmdet.registry", TASK_UTILS=TASK_UTILS)
    mod("mmdet.models"), mod("mmdet.models.task_modules"), mod("mmdet.models.task_modules.assigners")
    mod("mmdet.models.task_modules.assigners.assign_result", AssignResult=AssignResult)
    mod("mmdet.models.task_modules.assigners.base_assigner", BaseAssigner=BaseAssigner)
    mod("mmdet.structures"), mod("mmdet.structures.bbox", HorizontalBoxes=HorizontalBoxes, bbox_overlaps=bbox_overlaps, get_box_tensor=get_box_tensor)
    mod("mmrotate"), mod("mmrotate.structures")
    mod("mmrotate.structures.bbox", QuadriBoxes=QuadriBoxes, RotatedBoxes=RotatedBoxes, fake_rbbox_overlaps=fake_rbbox_overlaps, rbbox_overlaps=rbbox_overlaps)
    mod("mmrotate.models"), mod("mmrotate.models.task_modules"), mod("mmrotate.models.task_modules.assigners")
    mod("mmrotate.models.task_modules.assigners.rotate_iou2d_calculator", cast_tensor_type=cast_tensor_type)


def _load():
    _install_stubs()
    spec = importlib.util.spec_from_file_location("ref_max_iou_assigner", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.MTP_RD_MaxIoUAssigner


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


def main():
    Assigner = _load()
    out, sets = {}, {}
    for kind in R.KINDS:
        seed = C.first_seed(lambda s: C._assign_try(K, N, s, kind), lambda t: C.assign_condition(R.overlaps(t[0], t[1], kind)))
        gts, priors, labels = C._assign_try(K, N, seed, kind)
        assert gts.dtype == priors.dtype == np.float32
        sets[kind] = (gts, priors, labels)
        out[kind + ".gts"], out[kind + ".priors"], out[kind + ".labels"], out[kind + ".seed"] = gts, priors, labels, np.array(seed)
    for cfg, kind in RUNS:
        gts, priors, labels = sets[kind]
        a = Assigner(iou_calculator=dict(type=CALCULATOR[kind]), **C.ASSIGN_CFGS[cfg])
        res = a.assign(InstanceData(priors=torch.from_numpy(priors).double()),
                       InstanceData(rboxes=torch.from_numpy(gts).double(), rlabels=torch.from_numpy(labels)))
        p = "%s.%s." % (cfg, kind)
        out[p + "gt_inds"], out[p + "max_overlaps"], out[p + "labels"] = res.gt_inds.numpy(), res.max_overlaps.numpy(), res.labels.numpy()
        assert res.num_gts == K and res.max_overlaps.dtype == torch.float64
    path = os.path.join(HERE, "f21_box_ops.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
