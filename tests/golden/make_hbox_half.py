"""Generate f26_hbox_half.npz: the reference's own box half of Mask R-CNN (Multi-Task_Pretrain/instance_segmentation: rpn_head.py, base_bbox_head.py,
bbox_head.py, roi_head.py) run in float64 on the inputs of tests/hbox_cases.py.

Runs in the development container only (the reference is not on the GPU machine).  The files are imported by path as one package, with the STUB
method of make_oriented_rpn.py / make_oriented_roi.py (whose stubs are reused): what they import from mmcv / mmengine / mmdet is restated below
from the published algorithm and labelled STUB.  The STUB arithmetic calls tests/hbox_ref.py, tests/box_ref.py and tests/mask_ref.py in float64 --
RoIAlign (an autograd function over mask_ref's forward and backward), the coder, the overlaps, NMS -- or, for the losses and the accuracy, restates
the formulas in torch so that autograd gives the gradients.  mmdet's AnchorHead, the base class of MTP_IS_RPNHead, is not installed: the reference's
own copy of the same control flow, rotated_detection/anchor_head.py (MTP_RD_AnchorHead), is loaded by path in its place; its assigner and sampler
(rotated_detection/max_iou_assigner.py, random_sampler.py) stand in for mmdet's MaxIoUAssigner and RandomSampler and read the gts through their
.rboxes / .rlabels fields, which here carry the horizontal boxes.  That the copy is the same control flow on the horizontal case is what this
script checks: every recorded quantity is asserted against the float64 restatement of tests/hbox_cases.py before it is written.

The control flow is the reference's own code: MTP_IS_RPNHead.forward -> loss_by_feat (get_targets, _get_targets_single, loss_by_feat_single) and
predict_by_feat (_predict_by_feat_single, _bbox_post_process); MTP_IS_StandardRoIHead.gen_sampling_results -> train_bbox_forward -> the head's
forward -> external nn.Linear fc_cls / fc_reg -> bbox_loss (loss_and_target, get_targets, loss: the target of the box loss is the all-ones weight
tensor, base_bbox_head.py:430-435), and test_bbox_generate_roi -> test_bbox_roi_feats -> predict_bbox -> predict_by_feat -> _predict_by_feat_single.

Recorded per case of hbox_cases.SHAPES: a digest of the float32 inputs (the inputs themselves are hbox_cases.case(name)), the sampled indices of
every image, the RPN's and the box head's regression targets (the reference's get_targets) and the box head's labels, the per-level RPN losses, the
box head's losses and acc, the gradients of every parameter and (subsampled, every 3rd element) of every
map, and the kept proposals and detections of every image in output order for two configurations each.  The thresholds' margins of
hbox_cases.condition are asserted.  Fixed time stamps: the archive regenerates bit for bit.

    python tests/golden/make_hbox_half.py [OUTPUT]
"""
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
import hbox_cases as C  # noqa: E402
import hbox_ref as R  # noqa: E402
import make_box_ops as MB  # noqa: E402
import make_oriented_roi as MO  # noqa: E402
import make_oriented_rpn as MR  # noqa: E402

REG, ConfigDict, InstanceData = MR.REG, MR.ConfigDict, MO.InstanceData
REF_DIR = os.path.join(os.path.dirname(MR.REF_DIR), "instance_segmentation")
KEPT = []      # the candidate indices of every multiclass_nms call, in call order
THIN = 3       # the gradient maps are recorded every THIN-th element


# ---------------------------------------------------------------------------------------------------------------- STUBS
def batched_nms(boxes, scores, idxs, nms_cfg, class_agnostic=False):
    """STUB of mmcv.ops.batched_nms (type 'nms'): greedy NMS within each id, descending score"""
    cfg = dict(nms_cfg)
    assert cfg.pop("type", "nms") == "nms" and not class_agnostic
    keep = torch.from_numpy(BR.nms(boxes.numpy(), scores.numpy(), cfg["iou_threshold"], idxs.numpy()))
    return torch.cat([boxes[keep], scores[keep, None]], 1), keep


def multiclass_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None, return_inds=False, box_dim=4):
    """STUB of mmdet.models.layers.multiclass_nms"""
    num_classes = multi_scores.size(1) - 1
    bboxes = multi_bboxes.view(multi_scores.size(0), -1, box_dim)
    assert bboxes.shape[1] == num_classes and score_factors is None and not return_inds
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


def scale_boxes(boxes, scale_factor):
    """STUB of mmdet.structures.bbox.scale_boxes on a plain tensor"""
    return boxes * boxes.new_tensor(list(scale_factor)).repeat(boxes.size(-1) // 2)


def get_box_wh(boxes):
    """STUB of mmdet.structures.bbox.get_box_wh on a plain tensor"""
    return boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]


def unpack_gt_instances(batch_data_samples):
    """STUB of mmdet.models.utils.unpack_gt_instances"""
    return [s.gt_instances for s in batch_data_samples], [None for _ in batch_data_samples], [s.metainfo for s in batch_data_samples]


class SamplingResult(MO.SamplingResult):
    """STUB of mmdet's SamplingResult on boxes of four columns"""

    def __init__(self, pos_inds, neg_inds, priors, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.num_pos, self.num_neg = max(pos_inds.numel(), 1), max(neg_inds.numel(), 1)
        self.avg_factor = pos_inds.numel() + neg_inds.numel()
        self.pos_priors, self.neg_priors = priors[pos_inds], priors[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        self.pos_gt_labels = assign_result.labels[pos_inds]
        gt = MB.get_box_tensor(gt_bboxes)
        self.pos_gt_bboxes = gt.view(-1, 4)[self.pos_assigned_gt_inds.long()] if gt.numel() else gt.view(-1, 4)


@REG.register_module()
class HDeltaXYWHBBoxCoder:
    """STUB of mmdet's DeltaXYWHBBoxCoder (clip_border, no centre clamp): hbox_ref in float64"""
    encode_size = 4

    def __init__(self, target_means, target_stds, clip_border=True):
        assert clip_border
        self.means, self.stds = target_means, target_stds

    def encode(self, bboxes, gt_bboxes):
        return torch.from_numpy(R.encode(MR._np(bboxes), MR._np(gt_bboxes), self.means, self.stds))

    def decode(self, bboxes, pred_bboxes, max_shape=None, wh_ratio_clip=16 / 1000):
        ms = None if max_shape is None else tuple(int(v) for v in max_shape[:2])
        return torch.from_numpy(R.decode(MR._np(bboxes), MR._np(pred_bboxes), self.means, self.stds, ms, wh_ratio_clip))


@REG.register_module()
class HL1Loss(nn.Module):
    """STUB of mmdet's L1Loss: sum |pred - target| (weighted) / avg_factor"""

    def __init__(self, loss_weight=1.0):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override is None and avg_factor is not None
        if target.numel() == 0:
            return pred.sum() * 0
        loss = (pred - target).abs()
        if weight is not None:
            loss = loss * weight
        return loss.sum() / avg_factor * self.loss_weight


@REG.register_module()
class HSingleRoIExtractor(nn.Module):
    """STUB of mmdet's SingleRoIExtractor over mmcv's RoIAlign (7 x 7, adaptive grid, aligned): mask_ref in float64 through hbox_cases._Align"""

    def __init__(self, roi_layer, out_channels, featmap_strides, finest_scale=56):
        super().__init__()
        assert dict(roi_layer) == dict(type="RoIAlign", output_size=C.P, sampling_ratio=0) and tuple(featmap_strides) == C.ROI_STRIDES and finest_scale == C.FINEST
        self.num_inputs, self.out_channels = len(featmap_strides), out_channels

    def forward(self, feats, rois, roi_scale_factor=None):
        r = rois.detach().numpy()
        return C._Align.apply(r, np.ones(len(r), bool), np.float64, *feats[:self.num_inputs])


def _install_stubs():
    MO._install_stubs()

    def mod(name, **attrs):
        m = sys.modules.setdefault(name, types.ModuleType(name))
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    mod("mmcv.ops", batched_nms=batched_nms)
    mod("mmdet.models.task_modules.samplers", SamplingResult=SamplingResult)
    mod("mmdet.models.task_modules.samplers.sampling_result", SamplingResult=SamplingResult)
    mod("mmdet.structures.bbox", scale_boxes=scale_boxes, get_box_wh=get_box_wh, empty_box_as=MR._unused)
    mod("mmdet.models.utils", unpack_gt_instances=unpack_gt_instances)
    mod("mmdet.models.layers", multiclass_nms=multiclass_nms)
    REG.modules["BboxOverlaps2D"] = MB.BboxOverlaps2D
    REG.ALIAS = dict(REG.ALIAS, DeltaXYWHBBoxCoder="HDeltaXYWHBBoxCoder", L1Loss="HL1Loss", SingleRoIExtractor="HSingleRoIExtractor",
                     RandomSampler="HSeededRandomSampler")


def _load():
    """rotated_detection as ref_rd (anchor_head, assigner, sampler) and instance_segmentation as ref_is"""
    _install_stubs()
    for name, path in (("ref_rd", MR.REF_DIR), ("ref_is", REF_DIR)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    importlib.import_module("ref_rd.max_iou_assigner")
    sampler = importlib.import_module("ref_rd.random_sampler")

    @REG.register_module()
    class HSeededRandomSampler(sampler.MTP_RD_RandomSampler):
        """STUB: the reference's sampler with a reproducible random_choice -- hbox_cases.draw on a generator that main() seeds per case and stage"""
        draws = None

        def random_choice(self, gallery, num):
            assert len(gallery) >= num
            return torch.from_numpy(C.draw(type(self).draws, gallery.numpy(), num))
    anchor = importlib.import_module("ref_rd.anchor_head")
    m = sys.modules.setdefault("mmdet.models.dense_heads.anchor_head", types.ModuleType("mmdet.models.dense_heads.anchor_head"))
    m.AnchorHead = anchor.MTP_RD_AnchorHead      # STUB of mmdet's AnchorHead: the reference's copy of it
    importlib.import_module("ref_is.bbox_head")
    return importlib.import_module("ref_is.rpn_head").MTP_IS_RPNHead, importlib.import_module("ref_is.roi_head").MTP_IS_StandardRoIHead, HSeededRandomSampler


def close(a, b, tol=1e-9):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and (a.size == 0 or np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())), (a.shape, b.shape, np.abs(a - b).max() if a.size else 0)


def thin(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1)[::THIN])


def positions(scores, kept_scores):
    """scores are distinct (hbox_cases): the position of each kept one in the list"""
    if not len(kept_scores):
        return np.zeros(0, np.int64)
    pos = np.abs(np.asarray(scores)[None, :] - np.asarray(kept_scores)[:, None]).argmin(1)
    assert np.abs(np.asarray(scores)[pos] - kept_scores).max() < 1e-12 and len(set(pos.tolist())) == len(pos)
    return pos.astype(np.int64)


def main(path=None):
    Rpn, Roi, Sampler = _load()
    REG.ALIAS = {k: v for k, v in REG.ALIAS.items() if k != "CrossEntropyLoss"}      # the RPN's sigmoid loss: make_oriented_rpn's STUB under its own name
    rpn = Rpn(in_channels=C.C, feat_channels=C.FEAT,
              anchor_generator=dict(type="mmdet.AnchorGenerator", scales=list(C.SCALES), ratios=list(C.RATIOS), strides=list(C.STRIDES)),
              bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=list(C.RPN_MEANS), target_stds=list(C.RPN_STDS)),
              loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
              train_cfg=ConfigDict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlaps2D"), **C.RPN_ASSIGNER),
                                   sampler=dict(type="RandomSampler", num=C.RPN_NUM, pos_fraction=C.RPN_POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=False),
                                   allowed_border=-1, pos_weight=-1, debug=False),
              test_cfg=ConfigDict(C.PROPOSAL)).double()
    REG.ALIAS = dict(REG.ALIAS, CrossEntropyLoss="SoftmaxCrossEntropyLoss")      # from here on the RoI head's softmax loss (make_oriented_roi's STUB)
    roi = Roi(bbox_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=C.P, sampling_ratio=0), out_channels=C.C,
                                      featmap_strides=list(C.ROI_STRIDES)),
              bbox_head=dict(type="MTP_IS_Shared2FCBBoxHead", in_channels=C.C, fc_out_channels=C.FC_OUT, roi_feat_size=C.P,
                             bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=list(C.ROI_MEANS), target_stds=list(C.ROI_STDS)), reg_class_agnostic=False,
                             loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0)),
              train_cfg=ConfigDict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="BboxOverlaps2D"), **C.ROI_ASSIGNER),
                                   sampler=dict(type="RandomSampler", num=C.ROI_NUM, pos_fraction=C.ROI_POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=True),
                                   pos_weight=-1, debug=False),
              test_cfg=ConfigDict(C.RCNN)).double()
    fc_cls, fc_reg = nn.Linear(C.FC_OUT, C.K + 1).double(), nn.Linear(C.FC_OUT, 4 * C.K).double()
    out = {}
    for name in C.SHAPES:
        case, want = C.case(name), C.reference(name)
        assert C.condition(name, case), "the margins of hbox_cases.condition"
        p = name + "."
        out[p + "seed"] = np.array(C.SEEDS[name])
        out[p + "inputs_sha256"] = MO.digest(case["feats"] + case["gts"] + case["labels"] + [case[g][k] for g in ("rpn", "roi") for k in sorted(case[g])])
        gts = [InstanceData(bboxes=torch.from_numpy(g).double().reshape(-1, 4), labels=torch.from_numpy(l), rboxes=torch.from_numpy(g).double().reshape(-1, 4),
                            rlabels=torch.from_numpy(l)) for g, l in zip(case["gts"], case["labels"])]
        metas = [dict(img_shape=C.IMG + (3,), pad_shape=C.IMG + (3,), scale_factor=C.SCALE_FACTOR) for _ in gts]
        # ---- the RPN: the reference's flow
        rpn.load_state_dict({k: torch.from_numpy(v).double() for k, v in case["rpn"].items()})
        for q in rpn.parameters():
            q.grad = None
        x = [torch.from_numpy(f).double().requires_grad_() for f in case["feats"]]
        Sampler.draws = np.random.default_rng(C.SAMPLER_SEED + case["seed"])
        cls, reg = rpn(x)
        # (MTP_IS_RPNHead.loss_by_feat sets .labels to zero; the stand-in assigner reads .rlabels: they are zeroed for it the same way)
        rpn_gts = [InstanceData(bboxes=g.bboxes, labels=g.labels, rboxes=g.rboxes, rlabels=torch.zeros_like(g.rlabels)) for g in gts]
        got, inner = {}, rpn.get_targets

        def spy(*a, **k):
            got["targets"] = inner(*a, **k)
            return got["targets"]
        rpn.get_targets = spy
        losses = rpn.loss_by_feat(list(cls), list(reg), rpn_gts, metas)
        rpn.get_targets = inner
        rpn_targets = torch.cat(list(got["targets"][2]), 1).numpy()      # the reference's bbox_targets (images, anchors of all levels, 4)
        sum(losses["loss_rpn_cls"] + losses["loss_rpn_bbox"]).backward()
        w = want["rpn"]
        out[p + "rpn.loss_cls"], out[p + "rpn.loss_bbox"] = (np.array([float(v.detach()) for v in losses[k]]) for k in ("loss_rpn_cls", "loss_rpn_bbox"))
        close(out[p + "rpn.loss_cls"], w["loss_cls"]), close(out[p + "rpn.loss_bbox"], w["loss_bbox"])
        for b, sr in enumerate(rpn._raw_positive_infos["sampling_results"]):
            q = "%srpn.image%d." % (p, b)
            out[q + "pos_inds"], out[q + "neg_inds"], out[q + "pos_gt"] = sr.pos_inds.numpy(), sr.neg_inds.numpy(), sr.pos_assigned_gt_inds.numpy()
            assert out[q + "pos_inds"].tolist() == w["samples"][b]["pos"].tolist() and out[q + "neg_inds"].tolist() == w["samples"][b]["neg"].tolist()
            assert out[q + "pos_gt"].tolist() == w["samples"][b]["pos_gt"].tolist()
            out[q + "bbox_targets"] = rpn_targets[b][sr.pos_inds.numpy()]      # of the positives, in their order; zero elsewhere
            close(out[q + "bbox_targets"], w["targets"][b])
            assert not np.delete(rpn_targets[b], sr.pos_inds.numpy(), 0).any()
        for k, q in rpn.named_parameters():
            out[p + "rpn.grad." + k] = q.grad.numpy()
            close(q.grad.numpy(), w["G"][k])
        for l, f in enumerate(x):
            close(f.grad.numpy(), w["dfeats"][l])
            out["%srpn.level%d.dfeat" % (p, l)] = thin(f.grad.numpy())
        proposals = None
        for tag, min_size in (("prop", C.PROPOSAL["min_bbox_size"]), ("prop_all", -1)):
            cfg = ConfigDict(dict(C.PROPOSAL, min_bbox_size=min_size))
            res = rpn.predict_by_feat([m.detach() for m in cls], [m.detach() for m in reg], batch_img_metas=metas, cfg=cfg)
            for b, r in enumerate(res):
                ref = R.rpn_proposals([m[b] for m in w["cls"]], [m[b] for m in w["reg"]], C.priors(), C.SIZES, C.A, C.RPN_MEANS, C.RPN_STDS, C.IMG, cfg["nms_pre"],
                                      cfg["max_per_img"], cfg["nms"]["iou_threshold"], min_size)
                q = "%srpn.%s.image%d." % (p, tag, b)
                out[q + "keep"], out[q + "bboxes"], out[q + "scores"] = positions(ref[3][0], r.scores.numpy()), r.bboxes.numpy(), r.scores.numpy()
                assert out[q + "keep"].tolist() == ref[0].tolist() and int(r.labels.sum()) == 0
                close(r.bboxes.numpy(), ref[1]), close(r.scores.numpy(), ref[2])
            proposals = res if tag == "prop" else proposals
        # ---- the RoI head, training: the reference's flow on the float32-rounded proposals (what the next stage is handed in this project)
        with torch.no_grad():
            for k, v in case["roi"].items():
                owner = dict(roi.bbox_head.named_parameters()) if k.startswith("shared_fcs.") else dict(("fc_cls." + n, q) for n, q in fc_cls.named_parameters())
                owner = owner if k in owner else dict(("fc_reg." + n, q) for n, q in fc_reg.named_parameters())
                owner[k].copy_(torch.from_numpy(v).double())
        leaves = list(roi.bbox_head.parameters()) + list(fc_cls.parameters()) + list(fc_reg.parameters())
        for q in leaves:
            q.grad = None
        x = [torch.from_numpy(f).double().requires_grad_() for f in case["feats"]]
        boxes32 = [r.bboxes.numpy().astype(np.float32) for r in proposals]
        samples = [InstanceData(metainfo=m, gt_instances=g) for m, g in zip(metas, gts)]
        Sampler.draws = np.random.default_rng(2 * C.SAMPLER_SEED + case["seed"])
        sampling_results, _ = roi.gen_sampling_results((x, [InstanceData(bboxes=torch.from_numpy(b).double()) for b in boxes32], samples))
        bbox_feats, rois = roi.train_bbox_forward(x, sampling_results)
        x_cls, x_reg = roi.bbox_head(bbox_feats)
        results = dict(cls_score=fc_cls(x_cls), bbox_pred=fc_reg(x_reg), bbox_feats=bbox_feats)
        got, inner = {}, roi.bbox_head.get_targets

        def spy(*a, **k):
            got["targets"] = inner(*a, **k)
            return got["targets"]
        roi.bbox_head.get_targets = spy
        bl = roi.bbox_loss(C.K, sampling_results, rois, results)["loss_bbox"]
        roi.bbox_head.get_targets = inner
        (bl["loss_cls"] + bl["loss_bbox"]).backward()
        w = want["roi"]
        for b, sr in enumerate(sampling_results):
            q = "%sroi.image%d." % (p, b)
            out[q + "pos_inds"], out[q + "neg_inds"], out[q + "pos_gt"] = sr.pos_inds.numpy(), sr.neg_inds.numpy(), sr.pos_assigned_gt_inds.numpy()
            assert out[q + "pos_inds"].tolist() == w["samples"][b]["pos"].tolist() and out[q + "neg_inds"].tolist() == w["samples"][b]["neg"].tolist()
        # the reference's get_targets: labels and the encoded deltas of every sampled RoI, image after image (it computes them and its loss then
        # leaves them out: they are what reg_target='encoded' regresses to)
        labels, _, box_t, box_w = got["targets"]
        out[p + "roi.labels"], out[p + "roi.bbox_targets"], out[p + "roi.bbox_weights"] = labels.numpy(), box_t.numpy(), box_w.numpy().astype(np.int8)
        valid = w["lists"]["valid"]
        assert labels.numpy().tolist() == w["loss"]["encoded"]["labels"][valid].tolist()
        close(box_t.numpy(), w["loss"]["encoded"]["targets"][valid])
        assert (box_w.numpy().any(1) == (labels.numpy() < C.K)).all()
        for k in ("loss_cls", "loss_bbox", "acc"):      # the box loss as the reference computes it: towards the target 1
            out[p + "roi." + k] = np.array(float(bl[k].detach().reshape(-1)[0]))
            close(out[p + "roi." + k], w["loss"]["reference"][k])
        named = list(roi.bbox_head.named_parameters()) + [("fc_cls." + n, q) for n, q in fc_cls.named_parameters()] + [("fc_reg." + n, q) for n, q in fc_reg.named_parameters()]
        for k, q in named:
            g = q.grad.numpy() if q.grad is not None else np.zeros(tuple(q.shape))
            close(g, w["G"][k])
            out[p + "roi.grad." + k] = thin(g) if g.size > 4096 else g
        for l, f in enumerate(x[:len(C.ROI_STRIDES)]):
            g = f.grad.numpy() if f.grad is not None else np.zeros(tuple(f.shape))
            close(g, w["dfeats"][l])
            out["%sroi.level%d.dfeat" % (p, l)] = thin(g)
        # ---- the RoI head, test time: two configurations
        with torch.no_grad():
            xd = [f.detach() for f in x]
            props, trois = roi.test_bbox_generate_roi([InstanceData(bboxes=torch.from_numpy(b).double()) for b in boxes32])
            tfeats = roi.test_bbox_roi_feats(xd, trois)
            t_cls, t_reg = roi.bbox_head(tfeats)
            tres = dict(cls_score=fc_cls(t_cls), bbox_pred=fc_reg(t_reg))
            close(tres["cls_score"].numpy(), want["tcls"]), close(tres["bbox_pred"].numpy(), want["treg"])
            for tag, cfg, rescale in (("det", C.RCNN, False), ("det_rescale", C.RCNN, True)):
                del KEPT[:]
                dets = roi.predict_bbox(metas, dict(tres), props, trois, ConfigDict(cfg), C.K, rescale=rescale)
                assert len(KEPT) == len(dets) == C.BATCH
                for b, (d, kept) in enumerate(zip(dets, KEPT)):
                    ref = want["dets"]["rescale" if rescale else "plain"][b]
                    q = "%s%s.image%d." % (p, tag, b)
                    out[q + "keep"], out[q + "bboxes"], out[q + "scores"], out[q + "labels"] = kept.numpy(), d.bboxes.numpy(), d.scores.numpy(), d.labels.numpy()
                    assert kept.numpy().tolist() == ref[0].tolist() and d.labels.numpy().tolist() == ref[3].tolist()
                    close(d.bboxes.numpy(), ref[1]), close(d.scores.numpy(), ref[2])
    path = path or os.path.join(HERE, "f26_hbox_half.npz")
    MB.write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
