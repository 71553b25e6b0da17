"""Generate f22_oriented_rpn.npz: the reference's own oriented RPN head (Multi-Task_Pretrain/rotated_detection: rpn_head.py, anchor_head.py, dense_head.py,
random_sampler.py, max_iou_assigner.py) run in float64 on the inputs of tests/rpn_cases.py.

Runs in the development container only (the reference is not on the GPU machine).  The five files are imported by path as one package; what they
import from mmcv / mmengine / mmdet / mmrotate is not installed, so each of those is restated below from the published algorithm and labelled STUB
(those of make_box_ops.py are reused).  The STUB arithmetic calls tests/rpn_ref.py and tests/box_ref.py in float64 -- the anchor grid, the coder,
the overlaps, NMS -- or, for the two losses, restates rpn_ref's formulas in torch so that autograd gives the gradients.  The control flow is the
reference's own code: loss_by_feat, get_anchors, get_targets, _get_targets_single, loss_by_feat_single, the sampler's sample / _sample_pos /
_sample_neg, the assigner, predict_by_feat, _predict_by_feat_single and MTP_RD_OrientedRPNHead._bbox_post_process.  The STUB sampler's random_choice
takes the first `num` of a seeded numpy permutation.

Recorded per case of rpn_cases.SHAPES: the inputs (float32), the sampled indices of every image (into the anchors inside the image), the per-level
targets, the per-level losses, the gradients of their sum with respect to every map, and for two proposal configurations the kept proposals of
every image: their positions in the concatenated per-level top-nms_pre lists, boxes and scores, in output order.  Fixed time stamps: the archive
regenerates bit for bit.

    python tests/golden/make_oriented_rpn.py
"""
import functools
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
import box_ref as BR  # noqa: E402
import make_box_ops as MB  # noqa: E402
import rpn_cases as C  # noqa: E402
import rpn_ref as R  # noqa: E402

REF_DIR = "/root/reference/Multi-Task_Pretrain/rotated_detection"


def _np(t):
    return MB.get_box_tensor(t).detach().numpy()


# ---------------------------------------------------------------------------------------------------------------- STUBS
class InstanceData:
    """STUB of mmengine.structures.InstanceData: a bag of equally long fields that can be indexed together"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        vals = list(self.__dict__.values())
        return len(vals[0]) if vals else 0

    def __getitem__(self, item):
        return InstanceData(**{k: v[item] for k, v in self.__dict__.items()})


class ConfigDict(dict):
    """STUB of mmengine.config.ConfigDict: a dict whose keys read as attributes"""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError:
            raise AttributeError(k)
        return ConfigDict(v) if isinstance(v, dict) else v


class BaseModule(nn.Module):
    """STUB of mmengine.model.BaseModule"""

    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg


class Registry:
    """STUB of mmengine's Registry: scoped names ('mmdet.X') and the names the reference's configuration gives to its own MTP_RD_ classes"""
    ALIAS = {"MaxIoUAssigner": "MTP_RD_MaxIoUAssigner", "RBbox2HBboxOverlaps2D": "MTP_RD_RBbox2HBboxOverlaps2D", "RandomSampler": "SeededRandomSampler"}

    def __init__(self):
        self.modules = {}

    def register_module(self, *a, **k):
        def deco(cls):
            self.modules[cls.__name__] = cls
            return cls
        return deco

    def build(self, cfg, default_args=None):
        cfg = dict(cfg)
        name = cfg.pop("type").split(".")[-1]
        return self.modules[self.ALIAS.get(name, name)](**cfg, **(default_args or {}))


REG = Registry()


class RotatedBoxes(MB.RotatedBoxes):
    """STUB of mmrotate.structures.bbox.RotatedBoxes, as far as the post-processing reads it"""

    widths = property(lambda self: self.tensor[:, 2])
    heights = property(lambda self: self.tensor[:, 3])

    def __getitem__(self, item):
        return RotatedBoxes(self.tensor[item])

    def __len__(self):
        return self.tensor.shape[0]

    def numel(self):
        return self.tensor.numel()

    def empty_boxes(self):
        return RotatedBoxes(self.tensor.new_zeros(0, 5))


def get_box_wh(boxes):
    """STUB of mmdet.structures.bbox.get_box_wh"""
    if isinstance(boxes, MB._Boxes):
        return boxes.widths, boxes.heights
    return boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]


def rbox2hbox(t):
    """STUB of mmrotate.structures.bbox.rbox2hbox"""
    return torch.from_numpy(BR.rbox2hbox(t.numpy()))


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """STUB of mmcv.ops.batched_nms (type 'nms'): greedy NMS within each id, descending score"""
    cfg = dict(nms_cfg)
    assert cfg.pop("type", "nms") == "nms" and not class_agnostic
    keep = torch.from_numpy(BR.nms(boxes.numpy(), scores.numpy(), cfg["iou_threshold"], idxs.numpy()))
    return torch.cat([boxes[keep], scores[keep, None]], 1), keep


def _unused(*a, **k):
    """STUB of a symbol the reference imports and this run never calls"""
    raise NotImplementedError


def images_to_levels(target, num_levels):
    """STUB of mmdet.models.utils.images_to_levels"""
    target = torch.stack(target, 0)
    out, start = [], 0
    for n in num_levels:
        out.append(target[:, start:start + n])
        start += n
    return out


def multi_apply(func, *args, **kwargs):
    """STUB of mmdet.models.utils.multi_apply"""
    res = map(functools.partial(func, **kwargs) if kwargs else func, *args)
    return tuple(map(list, zip(*res)))


def unmap(data, count, inds, fill=0):
    """STUB of mmdet.models.utils.unmap"""
    ret = data.new_full((count,) + tuple(data.shape[1:]), fill)
    ret[inds.bool()] = data
    return ret


def select_single_mlvl(mlvl_tensors, batch_id, detach=True):
    """STUB of mmdet.models.utils.select_single_mlvl"""
    return [t[batch_id].detach() if detach else t[batch_id] for t in mlvl_tensors]


@REG.register_module()
class AnchorGenerator:
    """STUB of mmdet's AnchorGenerator (center_offset 0, scale_major): plain float64 tensors whatever use_box_type says"""

    def __init__(self, strides, ratios, scales, use_box_type=False):
        self.strides = [(s, s) for s in strides]
        self.base = [R.base_anchors(s, scales, ratios) for s in strides]
        self.num_base_priors = [len(b) for b in self.base]
        self.num_levels = len(strides)

    def grid_priors(self, featmap_sizes, dtype=None, device=None):
        return [torch.from_numpy(R.grid_priors(b, int(h), int(w), s)) for (h, w), s, b in zip(featmap_sizes, self.strides, self.base)]

    def valid_flags(self, featmap_sizes, pad_shape, device=None):
        return [torch.from_numpy(R.inside_flags(np.zeros((int(h) * int(w) * len(b), 4)), len(b), int(h), int(w), s, pad_shape[:2], pad_shape[:2], -1))
                for (h, w), s, b in zip(featmap_sizes, self.strides, self.base)]


def anchor_inside_flags(flat_anchors, valid_flags, img_shape, allowed_border=0):
    """STUB of mmdet's anchor_inside_flags"""
    img_h, img_w = img_shape[:2]
    if allowed_border < 0:
        return valid_flags
    a, b = flat_anchors, allowed_border
    return valid_flags & (a[:, 0] >= -b) & (a[:, 1] >= -b) & (a[:, 2] < img_w + b) & (a[:, 3] < img_h + b)


class SamplingResult:
    """STUB of mmdet's SamplingResult (avg_factor_with_neg)"""

    def __init__(self, pos_inds, neg_inds, priors, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.num_pos, self.num_neg = max(pos_inds.numel(), 1), max(neg_inds.numel(), 1)
        self.avg_factor = pos_inds.numel() + neg_inds.numel()
        self.pos_priors, self.neg_priors = priors[pos_inds], priors[neg_inds]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        self.pos_gt_labels = assign_result.labels[pos_inds]
        gt = MB.get_box_tensor(gt_bboxes)
        self.pos_gt_bboxes = gt.view(-1, 5)[self.pos_assigned_gt_inds.long()] if gt.numel() else gt.view(-1, 5)


@REG.register_module()
class MidpointOffsetCoder:
    """STUB of mmrotate's MidpointOffsetCoder ('le90'): rpn_ref in float64; decode returns boxes, as the published coder does"""
    encode_size = 6

    def __init__(self, target_means, target_stds, angle_version="le90"):
        assert angle_version == "le90"
        self.means, self.stds = target_means, target_stds

    def encode(self, bboxes, gt_bboxes):
        return torch.from_numpy(R.encode(_np(bboxes), _np(gt_bboxes), self.means, self.stds))

    def decode(self, bboxes, pred_bboxes, max_shape=None):
        return RotatedBoxes(torch.from_numpy(R.decode(_np(bboxes), _np(pred_bboxes), self.means, self.stds)))


@REG.register_module()
class CrossEntropyLoss(nn.Module):
    """STUB of mmdet's CrossEntropyLoss, use_sigmoid: rpn_ref's formula in torch; one class, label 0 is the object"""

    def __init__(self, use_sigmoid, loss_weight=1.0):
        super().__init__()
        assert use_sigmoid
        self.loss_weight = loss_weight

    def forward(self, cls_score, label, weight, avg_factor):
        z, t = cls_score.reshape(-1), (label == 0).to(cls_score.dtype)
        loss = (z.clamp(min=0) - z * t) + torch.log1p(torch.exp(-z.abs()))
        return (loss * weight.to(z.dtype)).sum() / avg_factor * self.loss_weight


@REG.register_module()
class SmoothL1Loss(nn.Module):
    """STUB of mmdet's SmoothL1Loss: rpn_ref's formula in torch"""

    def __init__(self, beta, loss_weight=1.0):
        super().__init__()
        self.beta, self.loss_weight = beta, loss_weight

    def forward(self, pred, target, weight, avg_factor):
        d = (pred - target).abs()
        loss = torch.where(d < self.beta, 0.5 * d * d / self.beta, d - 0.5 * self.beta)
        return (loss * weight).sum() / avg_factor * self.loss_weight


def _install_stubs():
    MB._install_stubs()

    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmcv"), mod("mmcv.cnn", ConvModule=_unused), mod("mmcv.ops", batched_nms=batched_nms)
    mod("mmengine.structures", InstanceData=InstanceData), mod("mmengine.config", ConfigDict=ConfigDict)
    mod("mmengine.model", BaseModule=BaseModule, constant_init=_unused)
    mod("mmdet.registry", MODELS=REG, TASK_UTILS=REG), mod("mmrotate.registry", MODELS=REG, TASK_UTILS=REG)
    mod("mmdet.structures", SampleList=list, DetDataSample=object, OptSampleList=list)
    mod("mmdet.structures.bbox", BaseBoxes=MB._Boxes, cat_boxes=lambda boxes, dim=0: torch.cat(list(boxes), dim), get_box_wh=get_box_wh,
        scale_boxes=_unused, empty_box_as=_unused)
    mod("mmdet.utils", **{k: object for k in ("ConfigType", "InstanceList", "OptConfigType", "OptInstanceList", "OptMultiConfig", "MultiConfig")})
    mod("mmdet.models.task_modules.prior_generators", AnchorGenerator=AnchorGenerator, anchor_inside_flags=anchor_inside_flags)
    mod("mmdet.models.task_modules.assigners", AssignResult=MB.AssignResult)
    mod("mmdet.models.task_modules.samplers", PseudoSampler=_unused)
    mod("mmdet.models.task_modules.samplers.sampling_result", SamplingResult=SamplingResult, ensure_rng=lambda rng=None: np.random.RandomState(0))
    mod("mmdet.models.utils", images_to_levels=images_to_levels, multi_apply=multi_apply, unmap=unmap, select_single_mlvl=select_single_mlvl,
        filter_scores_and_topk=_unused)
    mod("mmdet.models.test_time_augs", merge_aug_results=_unused), mod("mmdet.models.dense_heads", RPNHead=object)
    mod("mmrotate.structures.bbox", RotatedBoxes=RotatedBoxes, rbox2hbox=rbox2hbox)


def _load():
    """the reference's files as the package ref_rd (their relative imports resolve inside it; its __init__, which imports the whole detector, does
    not run)"""
    _install_stubs()
    pkg = types.ModuleType("ref_rd")
    pkg.__path__ = [REF_DIR]
    sys.modules["ref_rd"] = pkg
    importlib.import_module("ref_rd.max_iou_assigner")
    sampler = importlib.import_module("ref_rd.random_sampler")

    @REG.register_module()
    class SeededRandomSampler(sampler.MTP_RD_RandomSampler):
        """STUB: the reference's sampler with a reproducible random_choice -- the first `num` of a seeded permutation"""
        draws = np.random.default_rng(22)

        def random_choice(self, gallery, num):
            assert len(gallery) >= num
            return gallery[torch.from_numpy(self.draws.permutation(len(gallery))[:num])]
    return importlib.import_module("ref_rd.rpn_head").MTP_RD_OrientedRPNHead


def main():
    Head = _load()
    head = Head(in_channels=8, feat_channels=8,
                anchor_generator=dict(type="mmdet.AnchorGenerator", scales=list(C.SCALES), ratios=list(C.RATIOS), strides=list(C.STRIDES), use_box_type=True),
                bbox_coder=dict(type="MidpointOffsetCoder", angle_version="le90", target_means=list(C.MEANS), target_stds=list(C.STDS)),
                loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=C.BETA, loss_weight=1.0),
                train_cfg=ConfigDict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="mmrotate.RBbox2HBboxOverlaps2D"), **C.ASSIGNER),
                                     sampler=dict(type="RandomSampler", num=C.NUM, pos_fraction=C.POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=False),
                                     allowed_border=0, pos_weight=-1, debug=False),
                test_cfg=ConfigDict(C.PROPOSAL))
    out = {}
    for name in C.SHAPES:
        cls32, reg32, gts32 = C.case(name)
        img, pad, _ = C.SHAPES[name]
        L = len(cls32)
        cls = [torch.from_numpy(m).double().requires_grad_() for m in cls32]
        reg = [torch.from_numpy(m).double().requires_grad_() for m in reg32]
        gts = [InstanceData(rboxes=torch.from_numpy(g).double().reshape(-1, 5), rlabels=torch.zeros(len(g), dtype=torch.long)) for g in gts32]
        metas = [dict(img_shape=img + (3,), pad_shape=pad + (3,)) for _ in gts]
        got, inner = {}, head.get_targets

        def spy(*a, **k):
            got["targets"] = inner(*a, **k)
            return got["targets"]
        head.get_targets = spy
        losses = head.loss_by_feat(cls, reg, gts, metas)
        head.get_targets = inner
        sum(losses["loss_rpn_cls"] + losses["loss_rpn_bbox"]).backward()
        p = name + "."
        out[p + "seed"] = np.array(C.SEEDS[name])
        out[p + "loss_cls"], out[p + "loss_bbox"] = (np.array([float(v.detach()) for v in losses[k]]) for k in ("loss_rpn_cls", "loss_rpn_bbox"))
        labels, label_w, box_t, box_w, avg = got["targets"]
        out[p + "avg_factor"] = np.array(avg)
        for l in range(L):
            q = "%slevel%d." % (p, l)
            out[q + "cls"], out[q + "reg"] = cls32[l], reg32[l]
            out[q + "dcls"], out[q + "dreg"] = cls[l].grad.numpy(), reg[l].grad.numpy()
            out[q + "labels"], out[q + "label_weights"] = labels[l].numpy().astype(np.int8), label_w[l].numpy().astype(np.int8)
            out[q + "bbox_targets"], out[q + "bbox_weights"] = box_t[l].numpy(), box_w[l].numpy().astype(np.int8)
        for b, (g, sr) in enumerate(zip(gts32, head._raw_positive_infos["sampling_results"])):
            q = "%simage%d." % (p, b)
            out[q + "gts"] = g
            out[q + "pos_inds"], out[q + "neg_inds"], out[q + "pos_gt"] = sr.pos_inds.numpy(), sr.neg_inds.numpy(), sr.pos_assigned_gt_inds.numpy()
        priors, _, sizes = C.anchors(name)
        for tag, min_size in (("prop", C.PROPOSAL["min_bbox_size"]), ("prop_min", C.MIN_SIZE)):
            cfg = ConfigDict(dict(C.PROPOSAL, min_bbox_size=min_size))
            res = head.predict_by_feat([m.detach() for m in cls], [m.detach() for m in reg], batch_img_metas=metas, cfg=cfg)
            for b, r in enumerate(res):
                cb, rb = [m[b] for m in cls32], [m[b] for m in reg32]
                sc = R.decode_kept(cb, rb, priors, sizes, C.A, R.topk_per_level(cb, cfg["nms_pre"]), C.MEANS, C.STDS)[0]
                pos = np.abs(sc[None, :] - r.scores.numpy()[:, None]).argmin(1)      # scores are distinct (rpn_cases): the position of each kept one
                assert np.abs(sc[pos] - r.scores.numpy()).max() < 1e-12 and len(set(pos.tolist())) == len(pos)
                q = "%s%s.image%d." % (p, tag, b)
                out[q + "keep"], out[q + "bboxes"], out[q + "scores"] = pos.astype(np.int64), r.bboxes.tensor.numpy(), r.scores.numpy()
                assert int(r.labels.sum()) == 0 and len(r.labels) == len(pos) <= cfg["max_per_img"]
    path = os.path.join(HERE, "f22_oriented_rpn.npz")
    MB.write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
