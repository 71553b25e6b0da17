"""Generate f23_oriented_roi.npz: the reference's own oriented RoI head (Multi-Task_Pretrain/rotated_detection: standard_roi_head.py, bbox_head.py,
base_bbox_head.py, random_sampler.py, max_iou_assigner.py) run in float64 on the inputs of tests/roi_cases.py.

Runs in the development container only (the reference is not on the GPU machine).  The five files are imported by path as one package, with the
STUB method of make_oriented_rpn.py (whose stubs are reused): what they import from mmcv / mmengine / mmdet / mmrotate is restated below from the
published algorithm and labelled STUB.  The STUB arithmetic calls tests/roi_ref.py and tests/box_ref.py in float64 -- RoIAlignRotated (an autograd
function over roi_ref's forward and backward, so that the gradients reach the maps), the coder, the overlaps, NMS -- or, for the two losses and the
accuracy, restates the formulas in torch so that autograd gives the gradients.  The control flow is the reference's own code:
gen_sampling_results (the assigner, the sampler's sample with its add_gt_ step, _sample_pos / _sample_neg) -> train_bbox_forward -> the head's
forward -> external nn.Linear fc_cls / fc_reg -> bbox_loss (loss_and_target, get_targets, _get_targets_single, loss), and
test_bbox_generate_roi -> test_bbox_roi_feats -> predict_bbox -> predict_by_feat -> _predict_by_feat_single.  The STUB sampler's random_choice
takes the first `num` of a seeded numpy permutation (roi_cases.draw, one generator per case).

Recorded per case of roi_cases.SHAPES: digests of the float32 inputs (the inputs themselves are roi_cases.case(name)), the sampled indices of every
image (into [gts; proposals]), the rois, the RoI features, labels and targets, both losses and acc, the gradients of their sum with respect to
every map and parameter, the test scores and deltas, and for three test configurations the kept detections of every image (candidate indices
roi * K + class, boxes, scores, labels, in output order).  Fixed time stamps: the archive regenerates bit for bit.

    python tests/golden/make_oriented_roi.py [OUTPUT]
"""
import hashlib
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import box_ref as BR  # noqa: E402
import make_box_ops as MB  # noqa: E402
import make_oriented_rpn as MR  # noqa: E402
import roi_cases as C  # noqa: E402
import roi_ref as R  # noqa: E402

REG, ConfigDict = MR.REG, MR.ConfigDict
KEPT = []      # the candidate indices of every multiclass_nms call, in call order


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------- STUBS
class InstanceData(MR.InstanceData):
    """STUB of mmengine.structures.InstanceData: fields can be popped and tested for"""

    def pop(self, k):
        return self.__dict__.pop(k)

    def __contains__(self, k):
        return k in self.__dict__


def add_gt_(self, gt_labels):
    """STUB of mmdet's AssignResult.add_gt_: the gts become the first priors, each assigned to itself with overlap 1"""
    k = len(gt_labels)
    self.gt_inds = torch.cat([torch.arange(1, k + 1, dtype=torch.long), self.gt_inds])
    self.max_overlaps = torch.cat([self.max_overlaps.new_ones(k), self.max_overlaps])
    self.labels = torch.cat([gt_labels, self.labels])


class SamplingResult(MR.SamplingResult):
    """STUB of mmdet's SamplingResult: .priors is the positives followed by the negatives"""

    @property
    def priors(self):
        return torch.cat([self.pos_priors, self.neg_priors])


class BaseRoIHead(MR.BaseModule):
    """STUB of mmdet's BaseRoIHead: the constructor's order of calls and the with_* properties"""

    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None, shared_head=None, train_cfg=None, test_cfg=None,
                 init_cfg=None):
        super().__init__(init_cfg=init_cfg)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        assert shared_head is None and mask_head is None
        if bbox_head is not None:
            self.init_bbox_head(bbox_roi_extractor, bbox_head)
        self.init_assigner_sampler()

    with_bbox = property(lambda self: hasattr(self, "bbox_head") and self.bbox_head is not None)
    with_mask = property(lambda self: False)
    with_shared_head = property(lambda self: False)


def bbox2roi(bbox_list):
    """STUB of mmdet.structures.bbox.bbox2roi"""
    return torch.cat([torch.cat([MB.get_box_tensor(b).new_full((len(MB.get_box_tensor(b)), 1), i), MB.get_box_tensor(b)], 1) for i, b in enumerate(bbox_list)], 0)


def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """STUB of mmcv.ops.batched_nms (type 'nms_rotated'): greedy NMS within each id, descending score"""
    cfg = dict(nms_cfg)
    assert cfg.pop("type") == "nms_rotated" and not class_agnostic
    keep = torch.from_numpy(BR.nms(boxes.numpy(), scores.numpy(), cfg["iou_threshold"], idxs.numpy(), rotated=True))
    return torch.cat([boxes[keep], scores[keep, None]], 1), keep


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None, return_inds=False, box_dim=4):
    """STUB of mmdet.models.layers.multiclass_nms"""
    num_classes = multi_scores.size(1) - 1
    if multi_bboxes.shape[1] > box_dim:
        bboxes = multi_bboxes.view(multi_scores.size(0), -1, box_dim)
    else:
        bboxes = multi_bboxes[:, None].expand(multi_scores.size(0), num_classes, box_dim)
    scores = multi_scores[:, :-1]
    labels = torch.arange(num_classes, dtype=torch.long).view(1, -1).expand_as(scores)
    bboxes, scores, labels = bboxes.reshape(-1, box_dim), scores.reshape(-1), labels.reshape(-1)
    inds = (scores > score_thr).nonzero(as_tuple=False).squeeze(1)
    bboxes, scores, labels = bboxes[inds], scores[inds], labels[inds]
    if bboxes.numel() == 0:
        KEPT.append(inds)
        return torch.cat([bboxes, scores[:, None]], -1), labels
    dets, keep = batched_nms(bboxes, scores, labels, nms_cfg)
    if max_num > 0:
        dets, keep = dets[:max_num], keep[:max_num]
    KEPT.append(inds[keep])
    return dets, labels[keep]


def accuracy(pred, target, topk=1, thresh=None):
    """STUB of mmdet.models.losses.accuracy (top-1, percent)"""
    assert topk == 1 and thresh is None
    return (pred.argmax(1) == target).sum().to(pred.dtype).reshape(1) * (100.0 / pred.size(0))


@REG.register_module()
class SoftmaxCrossEntropyLoss(nn.Module):
    """STUB of mmdet's CrossEntropyLoss, use_sigmoid=False: roi_ref's formula in torch"""

    def __init__(self, use_sigmoid=False, loss_weight=1.0):
        super().__init__()
        assert not use_sigmoid
        self.loss_weight = loss_weight

    def forward(self, cls_score, label, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override is None
        m = cls_score.max(1, keepdim=True)[0]
        loss = (torch.log(torch.exp(cls_score - m).sum(1)) + m[:, 0]) - cls_score.gather(1, label[:, None])[:, 0]
        return (loss * weight.to(loss.dtype)).sum() / avg_factor * self.loss_weight


@REG.register_module()
class RoISmoothL1Loss(MR.SmoothL1Loss):
    """STUB of mmdet's SmoothL1Loss as the RoI head calls it"""

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override is None
        return super().forward(pred, target, weight, avg_factor)


@REG.register_module()
class DeltaXYWHTRBBoxCoder:
    """STUB of mmrotate's DeltaXYWHTRBBoxCoder ('le90', edge_swap, proj_xy): roi_ref in float64"""
    encode_size = 5

    def __init__(self, target_means, target_stds, angle_version="le90", norm_factor=None, edge_swap=True, proj_xy=True):
        assert angle_version == "le90" and norm_factor is None and edge_swap and proj_xy
        self.means, self.stds = target_means, target_stds

    def encode(self, bboxes, gt_bboxes):
        return torch.from_numpy(R.encode(MR._np(bboxes), MR._np(gt_bboxes), self.means, self.stds))

    def decode(self, bboxes, pred_bboxes, max_shape=None):
        return torch.from_numpy(R.decode(MR._np(bboxes), MR._np(pred_bboxes), self.means, self.stds))


class _Align(torch.autograd.Function):
    """roi_ref's RoIAlignRotated, forward and backward, in float64"""

    @staticmethod
    def forward(ctx, rois, *feats):
        ctx.rois, ctx.shapes = rois.numpy(), [tuple(f.shape) for f in feats]
        return torch.from_numpy(R.roi_align([f.detach().numpy() for f in feats], ctx.rois, C.STRIDES, C.P, C.S, C.CLOCKWISE, C.FINEST))

    @staticmethod
    def backward(ctx, dout):
        g = R.roi_align_bwd(dout.numpy(), ctx.shapes, ctx.rois, C.STRIDES, C.P, C.S, C.CLOCKWISE, C.FINEST)
        return (None,) + tuple(torch.from_numpy(a) for a in g)


@REG.register_module()
class RotatedSingleRoIExtractor(nn.Module):
    """STUB of mmrotate's RotatedSingleRoIExtractor over mmcv's RoIAlignRotated: roi_ref in float64 (level map included)"""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super().__init__()
        assert dict(roi_layer) == dict(type="RoIAlignRotated", out_size=C.P, sample_num=C.S, clockwise=C.CLOCKWISE)
        assert tuple(featmap_strides) == C.STRIDES and finest_scale == C.FINEST
        self.num_inputs, self.out_channels = len(featmap_strides), out_channels

    def forward(self, feats, rois, roi_scale_factor=None):
        return _Align.apply(rois.detach(), *feats)


def _install_stubs():
    MR._install_stubs()
    MB.AssignResult.add_gt_ = add_gt_
    mod = lambda name, **attrs: [setattr(sys.modules.setdefault(name, __import__("types").ModuleType(name)), k, v) for k, v in attrs.items()]      # noqa: E731
    mod("mmengine.structures", InstanceData=InstanceData)
    mod("mmdet.structures.bbox", bbox2roi=bbox2roi, get_box_tensor=MB.get_box_tensor, scale_boxes=MR._unused)
    mod("mmdet.models.task_modules.samplers", SamplingResult=SamplingResult)
    mod("mmdet.models.task_modules.samplers.sampling_result", SamplingResult=SamplingResult, ensure_rng=lambda rng=None: np.random.RandomState(0))
    mod("mmdet.models.utils", empty_instances=MR._unused, multi_apply=MR.multi_apply)
    mod("mmdet.models.roi_heads"), mod("mmdet.models.roi_heads.base_roi_head", BaseRoIHead=BaseRoIHead)
    mod("mmdet.models.layers", multiclass_nms=multiclass_nms), mod("mmdet.models.losses", accuracy=accuracy)
    REG.modules["RBboxOverlaps2D"] = MB.RBboxOverlaps2D
    REG.ALIAS = dict(MR.Registry.ALIAS, CrossEntropyLoss="SoftmaxCrossEntropyLoss", SmoothL1Loss="RoISmoothL1Loss", RandomSampler="RoISeededRandomSampler")


def _load():
    """the reference's files as the package ref_rd (make_oriented_rpn._load's way)"""
    _install_stubs()
    pkg = __import__("types").ModuleType("ref_rd")
    pkg.__path__ = [MR.REF_DIR]
    sys.modules["ref_rd"] = pkg
    importlib.import_module("ref_rd.max_iou_assigner")
    sampler = importlib.import_module("ref_rd.random_sampler")

    @REG.register_module()
    class RoISeededRandomSampler(sampler.MTP_RD_RandomSampler):
        """STUB: the reference's sampler with a reproducible random_choice -- roi_cases.draw on a generator that main() seeds per case"""
        draws = None

        def random_choice(self, gallery, num):
            assert len(gallery) >= num
            return torch.from_numpy(C.draw(type(self).draws, gallery.numpy(), num))
    importlib.import_module("ref_rd.bbox_head")
    return importlib.import_module("ref_rd.standard_roi_head").MTP_RD_StandardRoIHead, RoISeededRandomSampler


def main(path=None):
    Head, Sampler = _load()
    rcnn = dict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="mmrotate.RBboxOverlaps2D"), **C.ASSIGNER),
                sampler=dict(type="RandomSampler", num=C.NUM, pos_fraction=C.POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1, debug=False)
    head = Head(
        bbox_roi_extractor=dict(type="RotatedSingleRoIExtractor", roi_layer=dict(type="RoIAlignRotated", out_size=C.P, sample_num=C.S, clockwise=C.CLOCKWISE),
                                out_channels=C.C, featmap_strides=list(C.STRIDES)),
        bbox_head=dict(type="MTP_RD_Shared2FCBBoxHead", predict_box_type="rbox", in_channels=C.C, fc_out_channels=C.FC_OUT, roi_feat_size=C.P,
                       reg_predictor_cfg=dict(type="mmdet.Linear"), cls_predictor_cfg=dict(type="mmdet.Linear"),
                       bbox_coder=dict(type="mmrotate.DeltaXYWHTRBBoxCoder", angle_version="le90", norm_factor=None, edge_swap=True, proj_xy=True,
                                       target_means=C.MEANS, target_stds=C.STDS),
                       reg_class_agnostic=True, loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                       loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=C.BETA, loss_weight=1.0)),
        train_cfg=ConfigDict(rcnn), test_cfg=ConfigDict(C.RCNN)).double()
    fc_cls, fc_reg = nn.Linear(C.FC_OUT, C.K + 1).double(), nn.Linear(C.FC_OUT, 5).double()
    out = {}
    for name in C.SHAPES:
        case = C.case(name)
        img = C.SHAPES[name][0]
        params = dict(head.bbox_head.named_parameters())
        with torch.no_grad():
            for k, v in case["W"].items():
                owner = params if k.startswith("shared_fcs.") else dict(("fc_cls." + n, q) for n, q in fc_cls.named_parameters())
                owner = owner if k in owner else dict(("fc_reg." + n, q) for n, q in fc_reg.named_parameters())
                owner[k].copy_(torch.from_numpy(v).double())
        leaves = list(head.bbox_head.parameters()) + list(fc_cls.parameters()) + list(fc_reg.parameters())
        for q in leaves:
            q.grad = None
        x = [torch.from_numpy(f).double().requires_grad_() for f in case["feats"]]
        gts = [InstanceData(rboxes=torch.from_numpy(g).double().reshape(-1, 5), rlabels=torch.from_numpy(l)) for g, l in zip(case["gts"], case["labels"])]
        samples = [InstanceData(metainfo=dict(img_shape=img + (3,)), r_gt_instances=g) for g in gts]
        metas = [s.metainfo for s in samples]
        p = name + "."
        out[p + "seed"] = np.array(C.SEEDS[name])
        out[p + "inputs_sha256"] = digest(case["feats"] + case["gts"] + case["labels"] + case["props"] + [case["W"][k] for k in sorted(case["W"])])
        # ---- training: the reference's flow
        Sampler.draws = np.random.default_rng(C.SAMPLER_SEED + case["seed"])
        rpn = [InstanceData(bboxes=torch.from_numpy(q).double()) for q in case["props"]]
        sampling_results = head.gen_sampling_results((x, rpn, samples))
        bbox_feats, rois = head.train_bbox_forward(x, sampling_results)
        bbox_feats.retain_grad()
        x_cls, x_reg = head.bbox_head(bbox_feats)
        results = dict(cls_score=fc_cls(x_cls), bbox_pred=fc_reg(x_reg), bbox_feats=bbox_feats)
        spied, inner = {}, head.bbox_head.get_targets

        def spy(*a, **k):
            spied["targets"] = inner(*a, **k)
            return spied["targets"]
        head.bbox_head.get_targets = spy
        losses = head.bbox_loss(C.K, sampling_results, rois, results)["loss_bbox"]
        head.bbox_head.get_targets = inner
        (losses["loss_cls"] + losses["loss_bbox"]).backward()
        labels, label_w, box_t, box_w = spied["targets"]
        out[p + "rois"], out[p + "bbox_feats"], out[p + "d_bbox_feats"] = rois.detach().numpy(), bbox_feats.detach().numpy(), bbox_feats.grad.numpy().astype(np.float32)
        out[p + "cls_score"], out[p + "bbox_pred"] = results["cls_score"].detach().numpy(), results["bbox_pred"].detach().numpy()
        out[p + "labels"], out[p + "label_weights"] = labels.numpy(), label_w.numpy().astype(np.int8)
        out[p + "bbox_targets"], out[p + "bbox_weights"] = box_t.numpy(), box_w.numpy().astype(np.int8)
        for k in ("loss_cls", "loss_bbox", "acc"):
            out[p + k] = np.array(float(losses[k].detach().reshape(-1)[0]))
        for b, sr in enumerate(sampling_results):
            q = "%simage%d." % (p, b)
            out[q + "pos_inds"], out[q + "neg_inds"], out[q + "pos_gt"] = sr.pos_inds.numpy(), sr.neg_inds.numpy(), sr.pos_assigned_gt_inds.numpy()
        for l, f in enumerate(x):
            out["%slevel%d.dfeat" % (p, l)] = f.grad.numpy()
        for k, q in list(("" + n, q) for n, q in head.bbox_head.named_parameters()) + [("fc_cls." + n, q) for n, q in fc_cls.named_parameters()] + \
                [("fc_reg." + n, q) for n, q in fc_reg.named_parameters()]:
            out[p + "grad." + k] = q.grad.numpy()
        # ---- testing: the reference's flow, three configurations
        with torch.no_grad():
            xd = [f.detach() for f in x]
            rpn = [InstanceData(bboxes=torch.from_numpy(q).double()) for q in case["props"]]
            proposals, trois = head.test_bbox_generate_roi(rpn)
            tfeats = head.test_bbox_roi_feats(xd, trois)
            t_cls, t_reg = head.bbox_head(tfeats)
            tres = dict(cls_score=fc_cls(t_cls), bbox_pred=fc_reg(t_reg))
            out[p + "test.cls_score"], out[p + "test.bbox_pred"] = tres["cls_score"].numpy(), tres["bbox_pred"].numpy()
            for tag, cfg in (("det", C.RCNN), ("det_thr", C.RCNN_THR), ("det_cut", C.RCNN_CUT)):
                del KEPT[:]
                dets = head.predict_bbox(metas, dict(tres), proposals, trois, ConfigDict(cfg), C.K)
                assert len(KEPT) == len(dets) == C.BATCH
                for b, (d, kept) in enumerate(zip(dets, KEPT)):
                    q = "%s%s.image%d." % (p, tag, b)
                    out[q + "keep"], out[q + "bboxes"], out[q + "scores"], out[q + "labels"] = kept.numpy(), d.bboxes.numpy(), d.scores.numpy(), d.labels.numpy()
    path = path or os.path.join(HERE, "f23_oriented_roi.npz")
    MB.write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
