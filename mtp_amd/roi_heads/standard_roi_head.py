"""StandardRoIHead: the reference's MTP_RD_StandardRoIHead (rotated_detection/standard_roi_head.py; configured at oriented_rcnn.py:41-75, 100-128),
the second stage of Oriented R-CNN: RotatedSingleRoIExtractor -> Shared2FCBBoxHead -> softmax cross-entropy + SmoothL1 on DeltaXYWHTRBBoxCoder
targets, and multiclass NMS with nms_rotated at test time.

Everything between the proposals and the loss is fixed-size: per image `num` sample slots (positives, negatives, padding) with the counts on the
device, one RoIAlignRotated launch, three GEMMs, two loss launches, and back.  No host synchronisation on that path.  What is left on the host, in
predict: one synchronisation per batch for the numbers of candidates above score_thr, and one per image for the number of detections NMS kept."""
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import ops
from ..engine_decode import DecodeEngine
from ..registry import MODELS, TASK_UTILS
from ..task_modules.assign_result import AssignResult
from ..task_modules.iou_calculators import box_tensor
from ._cfg import field as _get, optional as _opt, strip_scope as _strip

F32 = torch.float32


@MODELS.register_module(name=["StandardRoIHead", "MTP_RD_StandardRoIHead"])
class StandardRoIHead(nn.Module):
    """StandardRoIHead(bbox_roi_extractor, bbox_head, train_cfg, test_cfg).  The bbox head may come without num_classes (pretraining): then
    num_classes, fc_cls and fc_reg are passed per call."""

    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None, shared_head=None, train_cfg=None, test_cfg=None,
                 init_cfg=None):
        super().__init__()
        me = type(self).__name__
        if mask_roi_extractor is not None or mask_head is not None:
            raise NotImplementedError("%s: %s" % (me, self.MASK_REFUSAL))
        if shared_head is not None:
            raise NotImplementedError("%s: a shared head is not built" % me)
        if bbox_roi_extractor is None or bbox_head is None:
            raise TypeError("%s: bbox_roi_extractor and bbox_head are needed" % me)
        self.bbox_roi_extractor = bbox_roi_extractor if isinstance(bbox_roi_extractor, nn.Module) else MODELS.build(_strip(bbox_roi_extractor, *self.SCOPES))
        self.bbox_head = bbox_head if isinstance(bbox_head, nn.Module) else MODELS.build(_strip(bbox_head, *self.HEAD_SCOPES))
        if self.bbox_roi_extractor.out_channels != self.bbox_head.in_channels or getattr(self.bbox_roi_extractor.roi_layers[0], self.ROI_SIZE) != self.bbox_head.roi_feat_size:
            raise ValueError("%s: the extractor's output is the bbox head's input" % me)
        self.train_cfg, self.test_cfg = (None if train_cfg is None else dict(train_cfg)), (None if test_cfg is None else dict(test_cfg))
        self.bbox_assigner = self.bbox_sampler = None
        self.add_gt_as_proposals = False
        if self.train_cfg is not None:
            if self.train_cfg.get("pos_weight", -1) > 0:
                raise NotImplementedError("%s: pos_weight > 0 is not built (every MTP configuration sets -1)" % me)
            self.bbox_assigner = TASK_UTILS.build(_strip(self.train_cfg["assigner"], "mmdet.", "mmrotate."))
            sampler = _strip(self.train_cfg.get("sampler", dict(type="RandomSampler", num=512, pos_fraction=0.25, add_gt_as_proposals=True)), "mmdet.")
            # the sampler class draws from what it is given; prepending the gts (the reference's add_gt_ step) is done here
            self.add_gt_as_proposals = bool(sampler.pop("add_gt_as_proposals", True))
            self.bbox_sampler = TASK_UTILS.build(dict(sampler, add_gt_as_proposals=False))

    with_bbox, with_mask, with_shared_head = True, False, False
    # what the horizontal box half (hbox_roi_head.HBoxRoIHead) has otherwise: the columns of a box (cx cy w h theta; there x1 y1 x2 y2), the scopes
    # stripped from the extractor's and the head's type, the RoI layer's attribute for its output size, the words of the mask refusal
    BOX_DIM, SCOPES, HEAD_SCOPES, ROI_SIZE, MASK_REFUSAL = 5, ("mmrotate.",), (), "out_size", "the mask branch is not built"

    def invalidate_weights(self):
        """the parameters were written through raw pointers (see Shared2FCBBoxHead.invalidate_weights)"""
        self.bbox_head.invalidate_weights()

    # ------------------------------------------------------------------ sampling
    def gen_sampling_results(self, rpn_results_list, batch_gt_instances=None, generator=None, sample_inds=None):
        """per image: assign the proposals, prepend the gts (add_gt_as_proposals: gt i gets gt_inds i + 1, overlap 1), sample `num` slots.
        rpn_results_list: per image .bboxes (n, 5) (or .priors) and optionally .count, a device scalar: only the first count rows are proposals.
        Also takes the reference's one argument (x, rpn_results_list, batch_gt_instances).  sample_inds: per image (pos_inds, neg_inds) into
        [gts; proposals], instead of the draw.
        -> dict(rois (images * num, 6), inds (images, num), sample_gt (images, num) rows of gts, n_pos, n_neg (images), gts (G, 5), gt_labels (G)).
        No host synchronisation."""
        if batch_gt_instances is None and isinstance(rpn_results_list, tuple) and len(rpn_results_list) == 3:
            _, rpn_results_list, batch_gt_instances = rpn_results_list
        if self.bbox_assigner is None:
            raise RuntimeError("%s: train_cfg (assigner, sampler) is needed for the loss" % type(self).__name__)
        if len(rpn_results_list) != len(batch_gt_instances):
            raise ValueError("%s: one list of proposals and one gt_instances per image" % type(self).__name__)
        S = self.bbox_sampler.num
        rois, inds, gt_rows, n_pos, n_neg, gts, labels, off = [], [], [], [], [], [], [], 0
        for b, (res, gt) in enumerate(zip(rpn_results_list, batch_gt_instances)):
            props = box_tensor(_get(res, "bboxes", "priors")).detach().to(F32).reshape(-1, self.BOX_DIM)
            dev = props.device
            boxes = box_tensor(_get(gt, "rboxes", "bboxes")).detach().to(device=dev, dtype=F32).reshape(-1, self.BOX_DIM)
            lab = _get(gt, "rlabels", "labels").to(device=dev, dtype=torch.int64).reshape(-1)
            count = _opt(res, "count")
            if count is not None:      # padding rows: never drawn, and harmless to the IoU kernel
                live = torch.arange(props.shape[0], device=dev) < count
                props = torch.where(live[:, None], props, torch.zeros_like(props))
            a = self.bbox_assigner.assign(SimpleNamespace(priors=props), SimpleNamespace(rboxes=boxes, rlabels=lab, bboxes=boxes, labels=lab))
            gt_inds = a.gt_inds if count is None else torch.where(live, a.gt_inds, torch.full_like(a.gt_inds, -1))
            K = boxes.shape[0]
            if self.add_gt_as_proposals and K:
                props = torch.cat([boxes, props])
                gt_inds = torch.cat([torch.arange(1, K + 1, device=dev), gt_inds])
            extra = {} if sample_inds is None else dict(pos_inds=sample_inds[b][0], neg_inds=sample_inds[b][1])
            sl = self.bbox_sampler.sample(AssignResult(K, gt_inds, None, None), generator=generator, **extra)
            n = props.shape[0]
            rows = props[sl.inds.clamp(0, max(n - 1, 0))] if n else torch.zeros(S, self.BOX_DIM, device=dev)
            rois.append(torch.cat([torch.full((S, 1), float(b), device=dev), rows], 1))
            inds.append(sl.inds)
            gt_rows.append(torch.where(sl.gt_inds >= 0, sl.gt_inds + off, sl.gt_inds))
            n_pos.append(sl.n_pos.reshape(()))
            n_neg.append(sl.n_neg.reshape(()))
            gts.append(boxes)
            labels.append(lab)
            off += K
        return dict(rois=torch.cat(rois).contiguous(), inds=torch.stack(inds), sample_gt=torch.stack(gt_rows).contiguous(), n_pos=torch.stack(n_pos),
                    n_neg=torch.stack(n_neg), gts=torch.cat(gts).contiguous(), gt_labels=torch.cat(labels).contiguous())

    # ------------------------------------------------------------------ RoI features
    def _levels(self, feats):
        """NCHW maps -> (rows per level (N H W, C) f32, triples, sizes, images)"""
        ex = self.bbox_roi_extractor
        feats = list(feats)[:ex.num_inputs]
        if len(feats) != ex.num_inputs or any(f.dim() != 4 or f.shape[1] != ex.out_channels for f in feats):
            raise ValueError("%s: expected %d NCHW maps of %d channels" % (type(self).__name__, ex.num_inputs, ex.out_channels))
        eng = DecodeEngine(self, "fp32")
        rows = [eng.to_rows(f.detach(), F32) for f in feats]
        sizes = [(int(f.shape[2]), int(f.shape[3])) for f in feats]
        return rows, [ops.rpn_map_rows(r, H, W) for r, (H, W) in zip(rows, sizes)], sizes, int(feats[0].shape[0])

    @torch.no_grad()
    def train_bbox_forward(self, x, sampling_results):
        """-> (bbox_feats (images * num, C, 7, 7), rois (images * num, 6)); the slots beyond n_pos + n_neg are zero"""
        s = sampling_results
        _, maps, sizes, images = self._levels(x)
        out = self.bbox_roi_extractor.extract(maps, sizes, images, s["rois"], valid=(s["n_pos"] + s["n_neg"]).contiguous())
        P = self.bbox_head.roi_feat_size
        return out.permute(0, 2, 1).reshape(out.shape[0], -1, P, P), s["rois"]

    def test_bbox_generate_roi(self, rpn_results_list):
        proposals = [box_tensor(_get(r, "bboxes", "priors")).detach().to(F32).reshape(-1, self.BOX_DIM) for r in rpn_results_list]
        rois = [torch.cat([p.new_full((p.shape[0], 1), float(b)), p], 1) for b, p in enumerate(proposals)]
        return proposals, torch.cat(rois).contiguous()

    def test_bbox_roi_feats(self, x, rois):
        return self.bbox_roi_extractor(list(x)[:self.bbox_roi_extractor.num_inputs], rois)

    def _bbox_forward(self, x, rois, num_classes=None, fc_cls=None, fc_reg=None):
        bbox_feats = self.test_bbox_roi_feats(x, rois)
        cls_score, bbox_pred = self.bbox_head(bbox_feats, num_classes, fc_cls, fc_reg)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, bbox_feats=bbox_feats)

    # ------------------------------------------------------------------ loss
    def _loss_rows(self, out, K, s, dout=None):
        h = self.bbox_head
        cls, reg = out[:, :K + 1], out[:, K + 1:K + 1 + ops.ROI_DELTAS]
        dcls = dreg = None
        if dout is not None:
            dcls, dreg = dout[:, :K + 1], dout[:, K + 1:K + 1 + ops.ROI_DELTAS]
        l = ops.roi_loss(cls, reg, K, s["rois"][:, 1:].contiguous(), s["gts"], s["gt_labels"], s["sample_gt"], s["n_pos"], s["n_neg"], h.bbox_coder.means,
                         h.bbox_coder.stds, h.beta, h.cls_weight, h.bbox_weight, dcls, dreg)
        return dict(loss_cls=l[0], loss_bbox=l[1], acc=l[2])

    @torch.no_grad()
    def bbox_loss(self, num_classes, sampling_results, rois, bbox_results):
        """the reference's signature: cls_score (images * num, K + 1) and bbox_pred (images * num, 5) of the sampled RoIs -> bbox_results with
        loss_bbox = dict(loss_cls, loss_bbox, acc)"""
        K = self.bbox_head.num_classes if num_classes is None else int(num_classes)
        cls, reg = bbox_results["cls_score"].detach().to(F32).contiguous(), bbox_results["bbox_pred"].detach().to(F32).contiguous()
        s = dict(sampling_results, rois=rois)
        h = self.bbox_head
        l = ops.roi_loss(cls, reg, K, rois[:, 1:].contiguous(), s["gts"], s["gt_labels"], s["sample_gt"], s["n_pos"], s["n_neg"], h.bbox_coder.means,
                         h.bbox_coder.stds, h.beta, h.cls_weight, h.bbox_weight)
        bbox_results = dict(bbox_results)
        bbox_results.update(loss_bbox=dict(loss_cls=l[0], loss_bbox=l[1], acc=l[2]))
        return bbox_results

    @torch.no_grad()
    def loss_and_grads(self, feats, rpn_results_list, batch_gt_instances, num_classes=None, fc_cls=None, fc_reg=None, generator=None, sample_inds=None):
        """one training pass without autograd -> (losses dict(loss_cls, loss_bbox, acc), {parameter name: gradient}, [d feats, NCHW f32]): the
        gradients of loss_cls + loss_bbox.  Parameter names: the bbox head's ('bbox_head.shared_fcs.0.weight', ...); predictors passed per call
        appear as 'fc_cls.*' / 'fc_reg.*'."""
        h, ex = self.bbox_head, self.bbox_roi_extractor
        s = self.gen_sampling_results(rpn_results_list, batch_gt_instances, generator, sample_inds)
        rows, maps, sizes, images = self._levels(feats)
        valid = (s["n_pos"] + s["n_neg"]).contiguous()
        x = ex.extract(maps, sizes, images, s["rois"], valid=valid)      # (the backward's entry launch works out the same levels again)
        R = x.shape[0]
        eng, out, c, K = h.forward_rows(x.view(R, -1), num_classes, fc_cls, fc_reg)
        dout = torch.zeros_like(out)
        losses = self._loss_rows(out, K, s, dout)
        _, fc, fr, names = h.predictors(num_classes, fc_cls, fc_reg)
        own = fc is getattr(h, "fc_cls", None)
        G = {n: torch.zeros_like(p) for n, p in h.named_parameters()}
        if not own:
            G.update({"fc_cls.weight": torch.zeros_like(fc.weight), "fc_cls.bias": torch.zeros_like(fc.bias), "fc_reg.weight": torch.zeros_like(fr.weight),
                      "fc_reg.bias": torch.zeros_like(fr.bias)})
        dx = eng.backward_rows(dout, c, G, names)
        grads = {("bbox_head." + n if (own or n.startswith("shared_fcs.")) else n): g for n, g in G.items()}
        drows = [torch.zeros_like(r) for r in rows]
        dmaps = [(d,) + m[1:] for d, m in zip(drows, maps)]
        ex.extract_bwd(dx.view(R, -1, ex.out_channels), dmaps, sizes, images, s["rois"], valid=valid)
        dfeats = [DecodeEngine.to_nchw(d, images, H, W) for d, (H, W) in zip(drows, sizes)]
        return losses, grads, dfeats

    def loss(self, x, rpn_results_list, batch_gt_instances, num_classes=None, fc_cls=None, fc_reg=None, generator=None, sample_inds=None):
        """-> dict(loss_cls, loss_bbox, acc), no gradients"""
        with torch.no_grad():
            s = self.gen_sampling_results(rpn_results_list, batch_gt_instances, generator, sample_inds)
            _, maps, sizes, images = self._levels(x)
            feats = self.bbox_roi_extractor.extract(maps, sizes, images, s["rois"], valid=(s["n_pos"] + s["n_neg"]).contiguous())
            _, out, _, K = self.bbox_head.forward_rows(feats.view(feats.shape[0], -1), num_classes, fc_cls, fc_reg)
            return self._loss_rows(out, K, s)

    # ------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict_bbox(self, x, batch_img_metas, rpn_results_list, rcnn_test_cfg=None, rescale=False, num_classes=None, fc_cls=None, fc_reg=None):
        """-> per image an object with bboxes (k, 5), scores (k), labels (k), descending score, and .keep (k): the (roi, class) candidates kept, as
        roi * num_classes + class with roi counted inside the image.  Host synchronisations: one per batch, for the numbers of candidates above
        score_thr, and one per image, for the number NMS kept.  At most 32 768 candidates per image (more raise)."""
        if rescale:
            raise NotImplementedError("%s: rescale is not built" % type(self).__name__)
        cfg = dict(self.test_cfg or {}) if rcnn_test_cfg is None else dict(rcnn_test_cfg)
        score_thr, max_per_img, nms_cfg = float(cfg.get("score_thr", 0.0)), int(cfg.get("max_per_img", -1)), dict(cfg["nms"])
        if nms_cfg.pop("type", "nms_rotated") != "nms_rotated":
            raise NotImplementedError("%s: the detections go through 'nms_rotated'" % type(self).__name__)
        thr = float(nms_cfg["iou_threshold"])
        h = self.bbox_head
        proposals, rois = self.test_bbox_generate_roi(rpn_results_list)
        K = h.predictors(num_classes, fc_cls, fc_reg)[0]
        dev = rois.device
        empty = lambda: SimpleNamespace(bboxes=torch.zeros(0, 5, device=dev), scores=torch.zeros(0, device=dev),      # noqa: E731
                                        labels=torch.zeros(0, dtype=torch.int64, device=dev), keep=torch.zeros(0, dtype=torch.int64, device=dev))
        if rois.shape[0] == 0:
            return [empty() for _ in proposals]
        _, maps, sizes, images = self._levels(x)
        feats = self.bbox_roi_extractor.extract(maps, sizes, images, rois)
        _, out, _, K = h.forward_rows(feats.view(feats.shape[0], -1), num_classes, fc_cls, fc_reg)
        scores, boxes, flags = ops.roi_predict(out[:, :K + 1], out[:, K + 1:K + 1 + ops.ROI_DELTAS], K, rois[:, 1:].contiguous(), h.bbox_coder.means,
                                               h.bbox_coder.stds, score_thr)
        # the candidates of multiclass_nms are the (roi, class) pairs above score_thr: per image they are sorted to the front (stable, descending
        # score), their number is read -- one synchronisation for the whole batch -- and only they go through NMS, with the class as the group
        ok = flags.bool()
        masked = torch.where(ok, scores, scores.new_full((), -1.0))
        bounds = [0]
        for p in proposals:
            bounds.append(bounds[-1] + p.shape[0])
        n_cand = torch.stack([ok[a:b].sum() for a, b in zip(bounds[:-1], bounds[1:])]).tolist()
        results = []
        for (a, b), n in zip(zip(bounds[:-1], bounds[1:]), n_cand):
            if n == 0:
                results.append(empty())
                continue
            ops.check_nms_count(n)
            sc = scores[a:b].reshape(-1)
            cand = torch.sort(masked[a:b].reshape(-1), descending=True, stable=True)[1][:n]      # roi * K + class, roi counted inside the image
            kept, count = ops.nms_sorted(boxes[a + cand // K].contiguous(), thr, (cand % K).contiguous(), True, max_per_img)
            sel = cand[kept[:int(count)]]      # the synchronisation of this image
            results.append(SimpleNamespace(bboxes=boxes[a + sel // K], scores=sc[sel], labels=sel % K, keep=sel))
        return results

    def predict(self, x, rpn_results_list, batch_img_metas=None, rescale=False, num_classes=None, fc_cls=None, fc_reg=None):
        return self.predict_bbox(x, batch_img_metas, rpn_results_list, self.test_cfg, rescale, num_classes, fc_cls, fc_reg)
