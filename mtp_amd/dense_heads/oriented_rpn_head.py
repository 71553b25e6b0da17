"""OrientedRPNHead: the reference's MTP_RD_OrientedRPNHead (rotated_detection/rpn_head.py, anchor_head.py; configured at oriented_rcnn.py:20-40, 77-99).

Training targets and both losses of the whole batch, forward and backward, are two launches (mtp_amd.ops.rpn_loss) fed by the fused assigner and the
synchronisation-free RandomSampler; the proposals of all images and levels are decoded by one launch (mtp_amd.ops.rpn_proposals) and then go through
the NMS kernels image by image.  The three convolutions run on engine_rpn.  What is left on the host: one synchronisation per new (feature-map
sizes, image shape) key, for the number of anchors inside the image, and one per image in predict_by_feat, for the number of proposals NMS kept."""
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import ops
from ..engine_rpn import RPNEngine
from ..registry import MODELS, TASK_UTILS
from ..task_modules.iou_calculators import box_tensor

F32 = torch.float32


def _type(cfg, *scopes):
    t = str(cfg.get("type"))
    for s in scopes:
        if t.startswith(s):
            return t[len(s):]
    return t


def _build(cfg, *scopes):
    cfg = dict(cfg)
    cfg["type"] = _type(cfg, *scopes)
    return TASK_UTILS.build(cfg)


def _get(obj, *names):
    for n in names:
        v = obj.get(n) if isinstance(obj, dict) else getattr(obj, n, None)
        if v is not None:
            return v
    raise AttributeError("none of %s in %r" % (", ".join(names), type(obj).__name__))


@MODELS.register_module(name=["OrientedRPNHead", "MTP_RD_OrientedRPNHead"])
class OrientedRPNHead(nn.Module):
    """OrientedRPNHead(in_channels, feat_channels=256, num_convs=1, anchor_generator, bbox_coder, loss_cls, loss_bbox, train_cfg, test_cfg,
    precision='fp32').  State dict: rpn_conv / rpn_cls / rpn_reg .weight / .bias.  One class, sigmoid scores."""

    # what the horizontal head (rpn_head.RPNHead) has otherwise: the deltas per anchor, the columns of a gt box, the scope of the coder's name
    DELTAS, BOX_DIM, CODER_SCOPES, CODER_NAME = ops.RPN_DELTAS, 5, ("mmrotate.",), "the midpoint-offset coder (six deltas)"

    def __init__(self, in_channels, feat_channels=256, num_convs=1, num_classes=1,
                 anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type="MidpointOffsetCoder", target_means=[0.0] * 6, target_stds=[1.0, 1.0, 1.0, 1.0, 0.5, 0.5]),
                 loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type="SmoothL1Loss", beta=1.0 / 9.0, loss_weight=1.0),
                 reg_decoded_bbox=False, train_cfg=None, test_cfg=None, precision="fp32", init_cfg=None):
        super().__init__()
        me = type(self).__name__
        if num_convs != 1:
            raise NotImplementedError("%s: num_convs > 1 is not built (no MTP configuration uses it)" % me)
        if num_classes != 1:
            raise NotImplementedError("%s: an RPN has one class" % me)
        if reg_decoded_bbox:
            raise NotImplementedError("%s: reg_decoded_bbox is not built" % me)
        if _type(loss_cls, "mmdet.") != "CrossEntropyLoss" or not loss_cls.get("use_sigmoid", False) or loss_cls.get("class_weight") is not None:
            raise NotImplementedError("%s: loss_cls %r is not built (CrossEntropyLoss, use_sigmoid=True, no class weights)" % (me, loss_cls))
        self._check_loss_bbox(loss_bbox)
        if loss_cls.get("reduction", "mean") != "mean" or loss_bbox.get("reduction", "mean") != "mean":
            raise NotImplementedError("%s: reduction other than 'mean' is not built" % me)
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        if in_channels % 8 or feat_channels % 8:
            raise ValueError("%s: in_channels and feat_channels must be multiples of 8 (the GEMM operands' rows are 16-byte chunks)" % me)
        self.in_channels, self.feat_channels, self.num_convs, self.precision = int(in_channels), int(feat_channels), 1, precision
        self.prior_generator = _build(anchor_generator, "mmdet.")
        self.bbox_coder = _build(bbox_coder, *self.CODER_SCOPES)
        if getattr(self.bbox_coder, "encode_size", None) != self.DELTAS:
            raise NotImplementedError("%s: the kernels are those of %s" % (me, self.CODER_NAME))
        A = set(self.prior_generator.num_base_priors)
        if len(A) != 1:
            raise ValueError("%s: every level has the same number of base anchors" % me)
        self.num_base_priors = A.pop()
        self.cls_weight, self.bbox_weight = float(loss_cls.get("loss_weight", 1.0)), float(loss_bbox.get("loss_weight", 1.0))
        self.beta = float(loss_bbox.get("beta", 1.0))
        self.train_cfg, self.test_cfg = (None if train_cfg is None else dict(train_cfg)), (None if test_cfg is None else dict(test_cfg))
        self.assigner = self.sampler = None
        if self.train_cfg is not None:
            if self.train_cfg.get("pos_weight", -1) > 0:
                raise NotImplementedError("%s: pos_weight > 0 is not built (every MTP configuration sets -1)" % me)
            self.assigner = _build(self.train_cfg["assigner"], "mmdet.", "mmrotate.")
            self.sampler = _build(self.train_cfg.get("sampler", dict(type="RandomSampler", num=256, pos_fraction=0.5, add_gt_as_proposals=False)), "mmdet.")
        self.rpn_conv = nn.Conv2d(self.in_channels, self.feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(self.feat_channels, self.num_base_priors, 1)
        self.rpn_reg = nn.Conv2d(self.feat_channels, self.num_base_priors * self.DELTAS, 1)
        for m in (self.rpn_conv, self.rpn_cls, self.rpn_reg):       # mmdet's init_cfg: Normal, std 0.01
            nn.init.normal_(m.weight, 0.0, 0.01)
            nn.init.constant_(m.bias, 0.0)
        self._inside, self._flat = {}, {}

    def _check_loss_bbox(self, loss_bbox):
        if _type(loss_bbox, "mmdet.") != "SmoothL1Loss" or not loss_bbox.get("beta", 1.0) > 0:
            raise NotImplementedError("%s: loss_bbox %r is not built (SmoothL1Loss, beta > 0)" % (type(self).__name__, loss_bbox))

    # ------------------------------------------------------------------ the convolutions
    def _params(self):
        return dict(self.named_parameters())

    def _check_feats(self, feats):
        feats = list(feats)
        if len(feats) != self.prior_generator.num_levels or any(f.dim() != 4 or f.shape[1] != self.in_channels for f in feats):
            raise ValueError("%s: expected %d NCHW maps of %d channels" % (type(self).__name__, self.prior_generator.num_levels, self.in_channels))
        return feats

    def _maps(self, feats):
        """-> (engine, rows (., ld) f32, context, cls maps, reg maps, sizes): the maps are views of `rows` by strides"""
        feats = self._check_feats(feats)
        eng = RPNEngine(self, self.precision)
        with torch.no_grad():
            out, c = eng.forward_maps(feats, self._params())
        A = self.num_base_priors
        sizes = [(H, W) for _, H, W in c["geoms"]]
        cls = [ops.rpn_map_rows(out, H, W, 0, r) for (H, W), r in zip(sizes, c["row0"])]
        reg = [ops.rpn_map_rows(out, H, W, A, r) for (H, W), r in zip(sizes, c["row0"])]
        return eng, out, c, cls, reg, sizes

    def _nchw(self, out, c):
        A, cls, reg = self.num_base_priors, [], []
        for (N, H, W), r in zip(c["geoms"], c["row0"]):
            m = RPNEngine.to_nchw(out[r:r + N * H * W], N, H, W)
            cls.append(m[:, :A].contiguous())
            reg.append(m[:, A:A * (1 + self.DELTAS)].contiguous())
        return cls, reg

    @torch.no_grad()
    def forward(self, feats):
        """feats: one NCHW map per level -> (cls_scores [(N, A, H, W)], bbox_preds [(N, DELTAS A, H, W)]) f32 (six deltas here, four in RPNHead).
        No autograd graph: training goes through loss_and_grads."""
        _, out, c, _, _, _ = self._maps(feats)
        return self._nchw(out, c)

    # ------------------------------------------------------------------ targets and loss
    def _flat_priors(self, sizes, device):
        """the priors of all levels as one (n, 4) tensor, kept per (sizes, device)"""
        key = (tuple(sizes), str(device))
        if key not in self._flat:
            self._flat[key] = torch.cat(self.prior_generator.grid_priors(sizes, device=device))
        return self._flat[key]

    def _anchors(self, sizes, meta, device):
        """-> (flat priors (n, 4), indices of the anchors inside the image) of one image; cached per key, one synchronisation per new key"""
        img = tuple(int(v) for v in meta["img_shape"][:2])
        pad = tuple(int(v) for v in meta.get("pad_shape", img)[:2])
        border = self.train_cfg.get("allowed_border", 0) if self.train_cfg else 0
        key = (tuple(sizes), pad, img, border, str(device))
        if key not in self._inside:
            lv = self.prior_generator.priors_and_flags(sizes, pad, img, border, device)
            self._inside[key] = torch.nonzero(torch.cat([f for _, f in lv])).squeeze(1)
        return self._flat_priors(sizes, device), self._inside[key]

    def get_samples(self, sizes, batch_gt_instances, batch_img_metas, device, generator=None, sample_inds=None):
        """assign and sample every image -> (flat priors (n, 4), gts of all images (K, 5), samples (images, num), sample_gt (images, num), n_pos (images),
        n_neg (images)): what mtp_amd.ops.rpn_loss reads.  No host synchronisation once the (sizes, shapes) key is known."""
        S = self.sampler.num
        rows, gt_rows, n_pos, n_neg, gts, off, flat = [], [], [], [], [], 0, None
        for b, (gt, meta) in enumerate(zip(batch_gt_instances, batch_img_metas)):
            flat, inside = self._anchors(sizes, meta, device)
            boxes = box_tensor(_get(gt, "rboxes", "bboxes")).detach().to(device=device, dtype=F32).reshape(-1, self.BOX_DIM)
            labels = _get(gt, "rlabels", "labels").to(device)
            res = self.assigner.assign(SimpleNamespace(priors=flat[inside]), SimpleNamespace(rboxes=boxes, rlabels=labels, bboxes=boxes, labels=labels))
            extra = {} if sample_inds is None else dict(pos_inds=sample_inds[b][0], neg_inds=sample_inds[b][1])
            sl = self.sampler.sample(res, generator=generator, **extra)
            if inside.numel():
                rows.append(inside[sl.inds.clamp(0, inside.numel() - 1)])
            else:
                rows.append(torch.zeros(S, dtype=torch.int64, device=device))
            gt_rows.append(torch.where(sl.gt_inds >= 0, sl.gt_inds + off, sl.gt_inds))
            n_pos.append(sl.n_pos.reshape(()))
            n_neg.append(sl.n_neg.reshape(()))
            gts.append(boxes)
            off += boxes.shape[0]
        return flat, torch.cat(gts).contiguous(), torch.stack(rows), torch.stack(gt_rows), torch.stack(n_pos), torch.stack(n_neg)

    def _loss(self, cls, reg, sizes, images, batch_gt_instances, batch_img_metas, device, grads, generator=None, sample_inds=None):
        if self.assigner is None:
            raise RuntimeError("%s: train_cfg (assigner, sampler) is needed for the loss" % type(self).__name__)
        if len(batch_gt_instances) != images or len(batch_img_metas) != images:
            raise ValueError("%s: one gt_instances and one img_meta per image" % type(self).__name__)
        flat, gts, samples, sample_gt, n_pos, n_neg = self.get_samples(sizes, batch_gt_instances, batch_img_metas, device, generator, sample_inds)
        dcls = dreg = None
        if isinstance(grads, tuple):       # one zeroed map per map
            dcls, dreg = [(g,) + m[1:] for g, m in zip(grads[0], cls)], [(g,) + m[1:] for g, m in zip(grads[1], reg)]
        elif grads is not None:            # one zeroed buffer in the layout of the buffer all maps are views of
            dcls, dreg = [(grads,) + m[1:] for m in cls], [(grads,) + m[1:] for m in reg]
        lc, lb = self._loss_op(cls, reg, sizes, flat, gts, samples, sample_gt, n_pos, n_neg, dcls, dreg)
        return dict(loss_rpn_cls=list(lc.unbind(0)), loss_rpn_bbox=list(lb.unbind(0)))

    def _loss_op(self, cls, reg, sizes, flat, gts, samples, sample_gt, n_pos, n_neg, dcls, dreg):
        return ops.rpn_loss(cls, reg, sizes, self.num_base_priors, flat, gts, samples, sample_gt, n_pos, n_neg, self.bbox_coder.means, self.bbox_coder.stds,
                            self.beta, self.cls_weight, self.bbox_weight, dcls, dreg)

    @torch.no_grad()
    def loss_by_feat(self, cls_scores, bbox_preds, batch_gt_instances, batch_img_metas, batch_gt_instances_ignore=None, generator=None, sample_inds=None,
                     return_grads=False):
        """cls_scores [(N, A, H, W)], bbox_preds [(N, DELTAS A, H, W)]; gt_instances with .rboxes (K, BOX_DIM) / .rlabels (K) (or .bboxes / .labels); img_metas
        with img_shape (and pad_shape).  sample_inds: per image (pos_inds, neg_inds) into the anchors inside the image, instead of the random draw.
        -> dict(loss_rpn_cls=[per level], loss_rpn_bbox=[per level]); with return_grads also the gradients of the sum of all losses with respect
        to cls_scores and bbox_preds, two lists of f32 maps"""
        cls = [ops.rpn_map_nchw(t.detach().to(F32).contiguous()) for t in cls_scores]
        reg = [ops.rpn_map_nchw(t.detach().to(F32).contiguous()) for t in bbox_preds]
        sizes = [(int(t.shape[2]), int(t.shape[3])) for t in cls_scores]
        images, device = int(cls_scores[0].shape[0]), cls_scores[0].device
        if not return_grads:
            return self._loss(cls, reg, sizes, images, batch_gt_instances, batch_img_metas, device, None, generator, sample_inds)
        dcls, dreg = ([ops._scratch(tuple(m[0].shape), device, F32).zero_() for m in maps] for maps in (cls, reg))
        losses = self._loss(cls, reg, sizes, images, batch_gt_instances, batch_img_metas, device, (dcls, dreg), generator, sample_inds)
        return losses, dcls, dreg

    @torch.no_grad()
    def loss_and_grads(self, feats, batch_gt_instances, batch_img_metas, generator=None, sample_inds=None):
        """one training pass without autograd -> (losses, {parameter name: gradient}, [d feats, NCHW f32]): the gradients of the sum of all losses"""
        eng, out, c, cls, reg, sizes = self._maps(feats)
        dout = ops._scratch(tuple(out.shape), out.device, F32).zero_()
        losses = self._loss(cls, reg, sizes, c["geoms"][0][0], batch_gt_instances, batch_img_metas, out.device, dout, generator, sample_inds)
        G = {n: torch.zeros_like(p) for n, p in self.named_parameters()}
        dxs = eng.backward_maps(dout, c, G)
        return losses, G, [RPNEngine.to_nchw(d, *g) for d, g in zip(dxs, c["geoms"])]

    # ------------------------------------------------------------------ proposals
    def _predict(self, cls, reg, score_rows, sizes, images, batch_img_metas, cfg, device):
        """score_rows[l]: (images, H W A) logits in anchor order, for the sort"""
        cfg = dict(self.test_cfg or {}) if cfg is None else dict(cfg)
        nms_pre, max_per_img, min_size = int(cfg.get("nms_pre", -1)), int(cfg["max_per_img"]), float(cfg.get("min_bbox_size", -1))
        nms_cfg = dict(cfg["nms"])
        if nms_cfg.pop("type", "nms") != "nms":
            raise NotImplementedError("%s: the proposals go through 'nms' on their circumscribed boxes" % type(self).__name__)
        thr = float(nms_cfg["iou_threshold"])
        flat = self._flat_priors(sizes, device)
        keep, counts = [], []
        for z in score_rows:
            n = z.shape[1]
            k = nms_pre if 0 < nms_pre < n else n
            keep.append(torch.sort(z, dim=1, descending=True, stable=True)[1][:, :k])
            counts.append(k)
        keep = torch.cat(keep, 1).contiguous()
        scores, rboxes, hboxes, level_ids, valid = self._proposals_op(cls, reg, sizes, flat, keep, counts, min_size, images, batch_img_metas, device)
        results = []
        for b in range(images):
            ok = valid[b].bool()
            order = torch.sort(torch.where(ok, scores[b], scores[b].new_full((), -1.0)), descending=True, stable=True)[1]      # the dropped boxes last
            kept, count = ops.nms_sorted(hboxes[b][order].contiguous(), thr, level_ids[b][order].contiguous(), False, max_per_img)
            n_valid = ok.sum()
            n = int(((kept < n_valid) & (torch.arange(kept.shape[0], device=device) < count)).sum())       # the host synchronisation of this image
            sel = order[kept[:n]]
            results.append(SimpleNamespace(bboxes=rboxes[b][sel], scores=scores[b][sel], labels=torch.zeros(n, dtype=torch.int64, device=device), keep=sel))
        return results

    def _proposals_op(self, cls, reg, sizes, flat, keep, counts, min_size, images, batch_img_metas, device):
        """-> (scores, the boxes of the results, the axis-aligned boxes NMS runs on, level ids, valid)"""
        return ops.rpn_proposals(cls, reg, sizes, self.num_base_priors, flat, keep, counts, self.bbox_coder.means, self.bbox_coder.stds, min_size)

    @torch.no_grad()
    def predict_by_feat(self, cls_scores, bbox_preds, batch_img_metas=None, cfg=None, rescale=False, with_nms=True):
        """-> per image an object with bboxes (n, 5) cx cy w h theta (RPNHead: (n, 4) x1 y1 x2 y2), scores (n), labels (n) zeros, descending score;
        .keep: their positions in the concatenated per-level top-nms_pre lists"""
        if rescale or not with_nms:
            raise NotImplementedError("%s: rescale and with_nms=False are not built (rpn_head.py asserts with_nms)" % type(self).__name__)
        cls = [ops.rpn_map_nchw(t.detach().to(F32).contiguous()) for t in cls_scores]
        reg = [ops.rpn_map_nchw(t.detach().to(F32).contiguous()) for t in bbox_preds]
        sizes = [(int(t.shape[2]), int(t.shape[3])) for t in cls_scores]
        images = int(cls_scores[0].shape[0])
        rows = [m[0].permute(0, 2, 3, 1).reshape(images, -1) for m in cls]
        return self._predict(cls, reg, rows, sizes, images, batch_img_metas, cfg, cls_scores[0].device)

    def _predict_rows(self, out, c, cls, reg, sizes, batch_img_metas, cfg):
        A, images = self.num_base_priors, c["geoms"][0][0]
        rows = [out[r:r + images * H * W, :A].reshape(images, H * W * A) for (H, W), r in zip(sizes, c["row0"])]
        return self._predict(cls, reg, rows, sizes, images, batch_img_metas, cfg, out.device)

    @torch.no_grad()
    def predict(self, feats, batch_img_metas=None, cfg=None):
        _, out, c, cls, reg, sizes = self._maps(feats)
        return self._predict_rows(out, c, cls, reg, sizes, batch_img_metas, cfg)

    @torch.no_grad()
    def loss_and_predict(self, feats, batch_gt_instances, batch_img_metas, proposal_cfg=None, generator=None, sample_inds=None):
        """-> (losses, per-image proposals) from one run of the convolutions; proposal_cfg defaults to test_cfg"""
        _, out, c, cls, reg, sizes = self._maps(feats)
        losses = self._loss(cls, reg, sizes, c["geoms"][0][0], batch_gt_instances, batch_img_metas, out.device, None, generator, sample_inds)
        return losses, self._predict_rows(out, c, cls, reg, sizes, batch_img_metas, proposal_cfg)


MTP_RD_OrientedRPNHead = OrientedRPNHead
