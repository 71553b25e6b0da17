"""Generate f18_seg_eval.npz: the reference's own sliding-window inference and IoU metric (Multi-Task_Pretrain/semantic_segmentation/encoder_decoder.py
MTP_SS_UperNet.slide_inference, metric.py MTP_SS_Metric.intersect_and_union / total_area_to_metrics).

Runs in the development container only (the reference is not on the GPU machine).  Both files are imported by path; what they import from mmseg /
mmengine / prettytable is not installed, so each of those is restated below and labelled STUB (none of it takes part in the recorded computations:
registries, type aliases, a base class that only stores its arguments, logging).

Recorded (arrays only):
  * slide_inference for a deterministic stand-in encode_decode that is a pure function of the crop -- a stride-4 conv to K channels with stored integer
    weights, resized bilinearly to the crop -- on integer images, in float64 (every value a multiple of 1 / 64, so the sums are exact), at the
    geometries of seg_eval_ref.F18_GEOMS: image 56 x 88, crop (32, 48), stride (24, 32) (the last column window clamped back to origin 40 over the one at 32: counts {1, 2, 3, 4, 6}) and image
    50 x 60, crop (32, 32), stride (12, 14) (stride < crop / 2: counts {1, 2, 3, 4, 6, 9});
  * intersect_and_union for three prediction / label pairs with 5 classes (ignored pixels; class 4 absent from both; one all-ignored label map) and
    total_area_to_metrics (fed the float64 sums) for the mIoU, mDice and mFscore families, nan_to_num None and 0, on the total of the three pairs and
    on the all-ignored pair alone (aAcc = 0 / 0).

    python tests/golden/make_seg_eval.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import seg_eval_ref as R  # noqa: E402  (the stand-in and the geometry table only: nothing recorded here comes from the restatement)

REF = "/root/reference/Multi-Task_Pretrain/semantic_segmentation"
K_SLIDE, K_METRIC = 2, 5


# ---------------------------------------------------------------------------------------------------------------- STUBS
class BaseSegmentor(nn.Module):
    """STUB of mmseg.models.segmentors.BaseSegmentor: what MTP_SS_UperNet's constructor and slide_inference touch"""

    def __init__(self, data_preprocessor=None, init_cfg=None):
        super().__init__()

    with_neck = property(lambda self: hasattr(self, "neck") and self.neck is not None)
    with_auxiliary_head = property(lambda self: hasattr(self, "auxiliary_head") and self.auxiliary_head is not None)
    with_decode_head = property(lambda self: hasattr(self, "decode_head") and self.decode_head is not None)


class _Registry:
    """STUB of mmseg.registry.MODELS: build() returns an object with the three attributes _init_decode_head reads"""

    def register_module(self, *a, **k):
        return lambda cls: cls

    def build(self, cfg):
        return types.SimpleNamespace(align_corners=False, num_classes=cfg["num_classes"], out_channels=cfg["num_classes"])


class BaseMetric:
    """STUB of mmengine.evaluator.BaseMetric"""

    def __init__(self, collect_device="cpu", prefix=None):
        self.results = []


def _install_stubs():
    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmseg"), mod("mmseg.registry", MODELS=_Registry())
    mod("mmseg.utils", ConfigType=dict, OptConfigType=dict, OptMultiConfig=dict, OptSampleList=list, SampleList=list,
        add_prefix=lambda d, p: {"%s.%s" % (p, k): v for k, v in d.items()})          # STUB of mmseg.utils
    mod("mmseg.models"), mod("mmseg.models.segmentors", BaseSegmentor=BaseSegmentor)
    mod("mmengine"), mod("mmengine.dist", is_main_process=lambda: True)               # STUB of mmengine.dist
    mod("mmengine.evaluator", BaseMetric=BaseMetric)
    mod("mmengine.logging", MMLogger=object, print_log=lambda *a, **k: None)          # STUB of mmengine.logging
    mod("mmengine.utils", mkdir_or_exist=lambda p: None)                              # STUB of mmengine.utils
    mod("prettytable", PrettyTable=object)                                            # STUB of prettytable


def _load(fname):
    spec = importlib.util.spec_from_file_location("ref_" + fname[:-3], os.path.join(REF, fname))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    _install_stubs()
    Seg, Metric = _load("encoder_decoder.py").MTP_SS_UperNet, _load("metric.py").MTP_SS_Metric
    out = {}
    g = torch.Generator().manual_seed(18)
    weight = torch.randint(-2, 3, (K_SLIDE, 3, 4, 4), generator=g).double()
    out["slide.weight"] = weight.numpy().astype(np.int8)
    for tag, (img, crop, stride) in R.F18_GEOMS.items():
        x = torch.randint(-3, 4, (1, 3, *img), generator=g).double()
        seg = Seg(decode_head=dict(type="STUB", num_classes=K_SLIDE), test_cfg=types.SimpleNamespace(mode="slide", stride=stride, crop_size=crop))
        seg.encode_decode = R.standin_encode_decode(weight, crop)
        y = seg.slide_inference(x, [dict()])
        out["slide.%s.input" % tag] = x.numpy().astype(np.int8)
        out["slide.%s.seg_logits" % tag] = y.numpy()
    # the metric
    H, W = 24, 32
    pairs = []
    for i, ignored in enumerate((0.15, 0.3, 1.0)):
        pred = torch.randint(0, K_METRIC - 1, (H, W), generator=g)
        lab = torch.randint(0, K_METRIC - 1, (H, W), generator=g)
        lab = torch.where(torch.rand(H, W, generator=g) < 0.6, pred, lab)       # a prediction that is mostly right
        lab[torch.rand(H, W, generator=g) < ignored] = 255
        areas = Metric.intersect_and_union(pred, lab, K_METRIC, 255)
        pairs.append(areas)
        out["metric.%d.pred" % i], out["metric.%d.label" % i] = pred.numpy().astype(np.uint8), lab.numpy().astype(np.uint8)
        for name, a in zip(("intersect", "union", "pred_label", "label"), areas):
            assert torch.equal(a, a.round())
            out["metric.%d.area_%s" % (i, name)] = a.long().numpy()
    totals = {"all": [sum(p[j] for p in pairs).double() for j in range(4)], "ignored": [pairs[2][j].double() for j in range(4)]}
    for tname, tot in totals.items():
        for fam in R.FAMILIES:
            for nan in (None, 0):
                ret = Metric.total_area_to_metrics(*tot, list(fam), nan, 1)
                for k, v in ret.items():
                    v = np.asarray(v)
                    assert v.dtype == np.float64
                    out["metric.%s.%s.%s.%s" % (tname, "+".join(fam), "nan" if nan is None else "zero", k)] = v
    path = os.path.join(HERE, "f18_seg_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
