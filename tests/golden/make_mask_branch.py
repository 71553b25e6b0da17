"""Generate f25_mask_branch.npz: the reference's own mask branch (Multi-Task_Pretrain/instance_segmentation: mask_head.py, roi_head.py) run in float64
on the inputs of tests/mask_cases.py.

Runs only where the reference's sources are present (they are not part of this repository; no test needs them).  The two files are imported by path as one package, with the STUB
method of make_oriented_roi.py: what they import from mmcv / mmengine / mmdet is restated below from the published algorithm and labelled STUB.  The
STUB arithmetic calls tests/mask_ref.py in float64 -- RoIAlign inside SingleRoIExtractor (an autograd function over mask_ref's forward and backward,
so that the gradients reach the maps) and inside BitmapMasks.crop_and_resize -- or, for the loss, restates the formula in torch so that autograd
gives the gradients.  The control flow is the reference's own code: train_mask_forward -> MTP_IS_FCNMaskHead.forward -> the external conv_logits ->
mask_loss (loss_and_target, get_targets, mask_target) as models.py:284-293 chains them, and predict_mask -> predict_by_feat ->
_predict_by_feat_single -> _do_paste_mask as models.py:295-307 does.  The reference pastes in float32 whatever the inputs (_do_paste_mask casts), so
the pasted values are recorded as it computes them, float32; everything else is float64.  Of the paste's two device branches the GPU one is
recorded (skip_empty=False, whole images; see main()).

Thresholds decide bits.  Before anything is written, every case's seed is searched again (mask_cases.search) and must be the pinned one, and no
float64 target average and no pasted value of any case may lie within mask_cases.MARGIN of its threshold: the GPU test can then compare every
target and every mask bit exactly.

Recorded per case of mask_cases.SHAPES: digests of the float32 inputs (the inputs themselves are mask_cases.case(name)), the head's state-dict keys,
the level of every positive, mask_feats, mask_preds, the pre-threshold target averages and the targets, loss_mask, the gradients of every map and
parameter, and for both paste frames and both thresholds the pasted masks (and, for 'base', the values before the threshold).  To stay under the
size limit of a committed file, mask_feats and mask_preds are recorded in full for 'base' and on every STEP-th row and column for the other cases;
the loss and the gradients, which depend on all of them, are always whole.  Fixed time stamps: the archive regenerates bit for bit.

    python tests/golden/make_mask_branch.py [OUTPUT]
"""
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_box_ops as MB  # noqa: E402
import make_oriented_rpn as MO  # noqa: E402
import mask_cases as C  # noqa: E402
import mask_ref as R  # noqa: E402

REF_DIR = os.path.join(os.path.dirname(MO.REF_DIR), "instance_segmentation")      # beside the rotated-detection package of make_oriented_rpn
REG = MO.Registry()
ConfigDict, InstanceData = MO.ConfigDict, MO.InstanceData
STEP = 2
AVGS = []      # the pre-threshold averages of every crop_and_resize call, in call order


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------- STUBS
class ConvModule(nn.Module):
    """STUB of mmcv.cnn.ConvModule without norm: conv (with bias) -> ReLU"""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, conv_cfg=None, norm_cfg=None):
        super().__init__()
        assert conv_cfg is None and norm_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding)
        self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.activate(self.conv(x))


def build_upsample_layer(cfg):
    """STUB of mmcv.cnn.build_upsample_layer: 'deconv' is nn.ConvTranspose2d"""
    cfg = dict(cfg)
    assert cfg.pop("type") == "deconv"
    return nn.ConvTranspose2d(**cfg)


def _unused(*a, **k):
    raise AssertionError("not part of the mask branch")


class BitmapMasks:
    """STUB of mmdet.structures.mask.BitmapMasks: masks (n, h, w) uint8; crop_and_resize is mask_ref in float64"""

    def __init__(self, masks, height, width):
        self.masks, self.height, self.width = np.asarray(masks, np.uint8).reshape(-1, height, width), height, width

    def crop_and_resize(self, bboxes, out_shape, inds, device="cpu", interpolation="bilinear", binarize=True):
        assert out_shape[0] == out_shape[1] and binarize and interpolation == "bilinear"
        avg, targets = R.mask_targets(bboxes, inds, self.masks, out_shape[0])
        AVGS.append(avg)
        return BitmapMasks(targets, *out_shape)

    def to_ndarray(self):
        return self.masks


def mask_target_single(pos_proposals, pos_assigned_gt_inds, gt_masks, cfg):
    """STUB of mmdet.structures.mask.mask_target_single"""
    mask_size = (cfg.mask_size, cfg.mask_size) if isinstance(cfg.mask_size, int) else tuple(cfg.mask_size)
    binarize = not cfg.get("soft_mask_target", False)
    if pos_proposals.size(0) == 0:
        return pos_proposals.new_zeros((0,) + mask_size).float()
    proposals_np = pos_proposals.detach().cpu().numpy().copy()
    maxh, maxw = gt_masks.height, gt_masks.width
    proposals_np[:, [0, 2]] = np.clip(proposals_np[:, [0, 2]], 0, maxw)
    proposals_np[:, [1, 3]] = np.clip(proposals_np[:, [1, 3]], 0, maxh)
    t = gt_masks.crop_and_resize(proposals_np, mask_size, device="cpu", inds=pos_assigned_gt_inds.cpu().numpy(), binarize=binarize).to_ndarray()
    return torch.from_numpy(t).float()


def mask_target(pos_proposals_list, pos_assigned_gt_inds_list, gt_masks_list, cfg):
    """STUB of mmdet.structures.mask.mask_target"""
    out = [mask_target_single(p, i, g, cfg) for p, i, g in zip(pos_proposals_list, pos_assigned_gt_inds_list, gt_masks_list)]
    return torch.cat(out)


@REG.register_module()
class CrossEntropyLoss(nn.Module):
    """STUB of mmdet's CrossEntropyLoss, use_mask=True (mask_cross_entropy): mask_ref's formula in torch"""

    def __init__(self, use_mask=False, loss_weight=1.0):
        super().__init__()
        assert use_mask
        self.loss_weight = loss_weight

    def forward(self, cls_score, label, class_label):
        z = cls_score[torch.arange(cls_score.size(0)), class_label]
        t = label.to(z.dtype)
        return ((z.clamp(min=0) - z * t) + torch.log1p(torch.exp(-z.abs()))).mean()[None] * self.loss_weight


class _Align(torch.autograd.Function):
    """mask_ref's RoIAlign over all levels, forward and backward, in float64"""

    @staticmethod
    def forward(ctx, rois, *feats):
        ctx.rois, ctx.shapes = rois.numpy(), [tuple(f.shape) for f in feats]
        return torch.from_numpy(R.roi_align([f.detach().numpy() for f in feats], ctx.rois, C.STRIDES, C.OUT, 0, True, C.FINEST)[0])

    @staticmethod
    def backward(ctx, dout):
        g = R.roi_align_bwd(dout.numpy(), ctx.shapes, ctx.rois, C.STRIDES, C.OUT, 0, True, C.FINEST)
        return (None,) + tuple(torch.from_numpy(a) for a in g)


@REG.register_module()
class SingleRoIExtractor(nn.Module):
    """STUB of mmdet's SingleRoIExtractor over mmcv's RoIAlign: mask_ref in float64 (level map included)"""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super().__init__()
        assert dict(roi_layer) == dict(type="RoIAlign", output_size=C.OUT, sampling_ratio=0)
        assert tuple(featmap_strides) == C.STRIDES and finest_scale == C.FINEST
        self.num_inputs, self.out_channels = len(featmap_strides), out_channels

    def forward(self, feats, rois, roi_scale_factor=None):
        if rois.shape[0] == 0:
            return feats[0].new_zeros(0, self.out_channels, C.OUT, C.OUT)
        return _Align.apply(rois.detach(), *feats)


@REG.register_module()
class NoAssigner:
    """STUB: the mask half takes sampling results as they are; the reference's constructor still builds an assigner and a sampler"""

    def __init__(self, **kw):
        pass


class BaseRoIHead(MO.BaseModule):
    """STUB of mmdet's BaseRoIHead: the constructor's order of calls and the with_* properties"""

    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None, shared_head=None, train_cfg=None, test_cfg=None,
                 init_cfg=None):
        super().__init__(init_cfg=init_cfg)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        assert shared_head is None and bbox_head is None
        if mask_head is not None:
            self.init_mask_head(mask_roi_extractor, mask_head)
        self.init_assigner_sampler()

    with_bbox = property(lambda self: False)
    with_mask = property(lambda self: hasattr(self, "mask_head") and self.mask_head is not None)
    with_shared_head = property(lambda self: False)


def bbox2roi(bbox_list):
    """STUB of mmdet.structures.bbox.bbox2roi"""
    return torch.cat([torch.cat([b.new_full((b.size(0), 1), i), b], 1) for i, b in enumerate(bbox_list)], 0)


def _install_stubs():
    def mod(name, **attrs):
        parts = name.split(".")
        for i in range(1, len(parts)):
            sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmcv.cnn", ConvModule=ConvModule, build_conv_layer=_unused, build_upsample_layer=build_upsample_layer)
    mod("mmcv.ops.carafe", CARAFEPack=type("CARAFEPack", (), {}))
    mod("mmengine.config", ConfigDict=ConfigDict), mod("mmengine.model", BaseModule=MO.BaseModule, ModuleList=nn.ModuleList)
    mod("mmengine.structures", InstanceData=InstanceData)
    mod("mmdet.registry", MODELS=REG, TASK_UTILS=REG)
    mod("mmdet.structures", SampleList=list, DetDataSample=object), mod("mmdet.structures.bbox", bbox2roi=bbox2roi)
    mod("mmdet.structures.mask", mask_target=mask_target)
    mod("mmdet.utils", **{k: object for k in ("ConfigType", "InstanceList", "OptConfigType", "OptMultiConfig")})
    mod("mmdet.models.task_modules.samplers", SamplingResult=object)
    mod("mmdet.models.utils", empty_instances=_unused, unpack_gt_instances=_unused)
    mod("mmdet.models.roi_heads.base_roi_head", BaseRoIHead=BaseRoIHead)


def _load():
    """the reference's files as the package ref_is (its __init__, which imports the whole detector, does not run)"""
    _install_stubs()
    pkg = types.ModuleType("ref_is")
    pkg.__path__ = [REF_DIR]
    sys.modules["ref_is"] = pkg
    importlib.import_module("ref_is.mask_head")
    return importlib.import_module("ref_is.roi_head").MTP_IS_StandardRoIHead


def thin(a, name):
    """what is recorded of mask_feats / mask_preds: all of it for 'base', every STEP-th row and column otherwise"""
    return a if name == "base" else np.ascontiguousarray(a[..., ::STEP, ::STEP])


def main():
    Head = _load()
    out = {"step": np.array(STEP)}
    for name in C.SHAPES:
        assert C.search(name) == C.SHAPES[name]["seed"], "the pinned seed of %s is the first whose margins hold" % name
        c = C.case(name)
        m_t, m_p = C.margins(c)
        assert m_t > C.MARGIN and m_p > C.MARGIN and C.level_margin(c) > 1e-3, (name, m_t, m_p)
        head = Head(mask_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=C.OUT, sampling_ratio=0), out_channels=c["C"],
                                            featmap_strides=list(C.STRIDES), finest_scale=C.FINEST),
                    mask_head=dict(type="MTP_IS_FCNMaskHead", num_convs=C.NUM_CONVS, in_channels=c["C"], conv_out_channels=C.CONV,
                                   loss_mask=dict(type="CrossEntropyLoss", use_mask=True, loss_weight=C.LOSS_WEIGHT)),
                    train_cfg=ConfigDict(assigner=dict(type="NoAssigner"), sampler=dict(type="NoAssigner"), mask_size=C.M, pos_weight=-1, debug=False),
                    test_cfg=ConfigDict(mask_thr_binary=C.THR)).double()
        p = name + "."
        out[p + "state_keys"] = np.array(sorted(head.state_dict()))
        head.mask_head.load_state_dict({k: torch.from_numpy(v).double() for k, v in c["weights"].items()})
        conv_logits = nn.Conv2d(C.CONV, C.K, 1).double()
        conv_logits.load_state_dict({k: torch.from_numpy(v).double() for k, v in c["conv_logits"].items()})
        feats = [torch.from_numpy(f).double().requires_grad_() for f in c["feats"]]
        samples = [types.SimpleNamespace(pos_priors=torch.from_numpy(q["boxes"]).double().reshape(-1, 4), pos_assigned_gt_inds=torch.from_numpy(q["gt"]),
                                         pos_gt_labels=torch.from_numpy(q["labels"]), neg_priors=torch.zeros(0, 4, dtype=torch.float64)) for q in c["pos"]]
        gts = [InstanceData(masks=BitmapMasks(c["bitmaps"][a:b], C.IMG, C.IMG)) for a, b in zip(c["gt_start"][:-1], c["gt_start"][1:])]
        # models.py:284-293
        del AVGS[:]
        mask_feats = head.train_mask_forward(feats, samples, None)
        mask_preds = conv_logits(head.mask_head(mask_feats))
        res = head.mask_loss(dict(mask_preds=mask_preds, mask_feats=mask_feats), samples, gts)
        loss = res["loss_mask"]["loss_mask"]
        loss.sum().backward()
        n = mask_feats.shape[0]
        rois = bbox2roi([s.pos_priors for s in samples]).numpy()
        out[p + "seed"] = np.array(C.SHAPES[name]["seed"])
        out[p + "digest"] = digest(c["feats"] + [c["bitmaps"], c["rois"], c["sample_gt"], c["labels"], c["n_pos"], c["paste"]["logits"], c["paste"]["boxes"]]
                                   + [c["weights"][k] for k in sorted(c["weights"])] + [c["conv_logits"][k] for k in sorted(c["conv_logits"])])
        out[p + "levels"] = R.map_roi_levels(rois, C.FINEST, len(C.STRIDES)).astype(np.int8) if n else np.zeros(0, np.int8)
        out[p + "mask_feats"], out[p + "mask_preds"] = thin(mask_feats.detach().numpy(), name), thin(mask_preds.detach().numpy(), name)
        avg = np.concatenate(AVGS) if AVGS else np.zeros((0, C.M, C.M))
        assert len(avg) == n and (n == 0 or float(np.abs(avg - 0.5).min()) > C.MARGIN)
        out[p + "target_avg"] = avg
        mt = head.mask_head.get_targets(samples, gts, head.train_cfg).numpy()
        assert np.array_equal(mt, (avg >= 0.5).astype(np.float32))
        out[p + "targets"] = mt.astype(np.uint8)
        out[p + "loss_mask"] = np.asarray(float(loss.sum().detach()))
        zero = lambda t: np.zeros(tuple(t.shape))      # noqa: E731
        for l, f in enumerate(feats):
            out["%slevel%d.dfeat" % (p, l)] = f.grad.numpy() if f.grad is not None else zero(f)
        for k, v in head.named_parameters():
            out[p + "grad." + k] = v.grad.numpy() if v.grad is not None else zero(v)
        for k, v in conv_logits.named_parameters():
            out[p + "grad.conv_logits." + k] = v.grad.numpy() if v.grad is not None else zero(v)
        # models.py:295-307; the reference pastes in float32
        q = c["paste"]
        ref_mod = sys.modules["ref_is.mask_head"]
        if not hasattr(ref_mod, "_paste_as_on_gpu"):
            # _predict_by_feat_single branches on the device: on a GPU it pastes whole images (skip_empty=False), on the CPU only the window
            # around the boxes (skip_empty=True), and the two differ for a degenerate box, whose infinite coordinates become 0 and paint whole
            # rows or columns.  What is built is the GPU branch, and this generator runs the reference on the CPU: the module's _do_paste_mask is made to take it.
            inner = ref_mod._do_paste_mask
            ref_mod._paste_as_on_gpu = inner
            ref_mod._do_paste_mask = lambda masks, boxes, img_h, img_w, skip_empty=True: inner(masks, boxes, img_h, img_w, skip_empty=False)
        for rescale, boxes, h, w in C.paste_frames(c):
            for thr in (C.THR, -1.0):
                head.test_cfg = ConfigDict(mask_thr_binary=thr)
                results = [InstanceData(bboxes=torch.from_numpy(q["boxes"][:4].copy()), labels=torch.from_numpy(q["labels"][:4])),
                           InstanceData(bboxes=torch.from_numpy(q["boxes"][4:].copy()), labels=torch.from_numpy(q["labels"][4:]))]
                metas = [dict(ori_shape=C.PASTE_HW, scale_factor=C.PASTE_SCALE)] * 2
                done = head.predict_mask(metas, results, dict(mask_preds=torch.from_numpy(q["logits"])), rescale=rescale)
                masks = torch.cat([r.masks for r in done]).numpy()
                assert masks.shape == (len(boxes), h, w)
                tag = "%spaste.%s.%s." % (p, "rescale" if rescale else "scaled", "bool" if thr >= 0 else "u8")
                out[tag + "masks"] = masks.astype(np.uint8)
                if rescale:
                    assert np.array_equal(torch.cat([r.bboxes for r in done]).numpy(), boxes)
            if name == "base":
                prob = torch.from_numpy(q["logits"]).sigmoid()[torch.arange(len(boxes)), torch.from_numpy(q["labels"])][:, None]
                vals = ref_mod._paste_as_on_gpu(prob, torch.from_numpy(boxes), h, w, skip_empty=False)[0].numpy()
                assert float(np.abs(vals.astype(np.float64) - C.THR).min()) > C.MARGIN
                out["%spaste.%s.values" % (p, "rescale" if rescale else "scaled")] = vals
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "f25_mask_branch.npz")
    MB.write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
