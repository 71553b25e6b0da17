"""HBoxRoIHead ('MTP_IS_BBoxRoIHead'): the box half of the reference's instance-segmentation RoI head (instance_segmentation/roi_head.py:
gen_sampling_results, train_bbox_forward, test_bbox_generate_roi, test_bbox_roi_feats, _bbox_forward, bbox_loss, predict_bbox; configured at
mask_rcnn.py:35-55, 92-108, 115-119): SingleRoIExtractor (RoIAlign 7, adaptive grid) -> MTP_IS_Shared2FCBBoxHead -> softmax cross-entropy + the
per-class L1, and multiclass NMS at test time.  The mask half is MaskRoIHead ('MTP_IS_StandardRoIHead'); the two compose through data:
gen_sampling_results returns the positives in the slot form MaskRoIHead.loss_and_grads takes, predict / predict_bbox return the result lists
MaskRoIHead.predict takes.

Everything between the proposals and the loss is fixed-size, as in StandardRoIHead: per image `num` sample slots (positives, negatives, padding)
with the counts on the device, one RoIAlign launch, three GEMMs, two loss launches, and back.  No host synchronisation on that path."""
import torch

from ..engine_decode import DecodeEngine
from ..registry import MODELS
from .standard_roi_head import StandardRoIHead

F32 = torch.float32


@MODELS.register_module(name=["MTP_IS_BBoxRoIHead"])
class HBoxRoIHead(StandardRoIHead):
    """HBoxRoIHead(bbox_roi_extractor, bbox_head, train_cfg, test_cfg).  The bbox head may come without num_classes (the reference's form): then
    num_classes, fc_cls and fc_reg are passed per call."""

    BOX_DIM, SCOPES, HEAD_SCOPES, ROI_SIZE = 4, ("mmdet.",), ("mmdet.",), "output_size"
    MASK_REFUSAL = "this class is the box half; the mask half is MTP_IS_StandardRoIHead"

    # ------------------------------------------------------------------ sampling
    def gen_sampling_results(self, rpn_results_list, batch_gt_instances=None, generator=None, sample_inds=None):
        """StandardRoIHead.gen_sampling_results on boxes (n, 4): rois (images * num, 5), inds, sample_gt, n_pos, n_neg, gts (G, 4), gt_labels (G).
        Beside the slots, 'pos': the positives in the slot form MaskRoIHead.loss_and_grads takes -- dict(boxes (images * num, 4), sample_gt (images,
        num), labels (images * num), n_pos (images)); the first n_pos[b] slots of image b are its positives.  No host synchronisation."""
        s = super().gen_sampling_results(rpn_results_list, batch_gt_instances, generator, sample_inds)
        G = s["gt_labels"].numel()
        rows = s["sample_gt"].reshape(-1).clamp(0, max(G - 1, 0))
        labels = s["gt_labels"][rows].contiguous() if G else rows.new_zeros(rows.shape)
        s["pos"] = dict(boxes=s["rois"][:, 1:].contiguous(), sample_gt=s["sample_gt"], labels=labels, n_pos=s["n_pos"])
        return s

    # ------------------------------------------------------------------ loss
    def _loss_rows(self, out, K, s, dout=None):
        h = self.bbox_head
        c0 = h.reg_col(K)
        dcls = dreg = None
        if dout is not None:
            dcls, dreg = dout[:, :K + 1], dout[:, c0:c0 + 4 * K]
        return h.loss_and_target(out[:, :K + 1], out[:, c0:c0 + 4 * K], s["rois"], s, K, dcls, dreg)["loss_bbox"]

    @torch.no_grad()
    def bbox_loss(self, num_classes, sampling_results, rois, bbox_results):
        """the reference's signature: cls_score (images * num, K + 1) and bbox_pred (images * num, 4 K) of the sampled RoIs -> bbox_results with
        loss_bbox = dict(loss_cls, loss_bbox, acc)"""
        K = self.bbox_head.num_classes if num_classes is None else int(num_classes)
        cls, reg = bbox_results["cls_score"].detach().to(F32).contiguous(), bbox_results["bbox_pred"].detach().to(F32).contiguous()
        bbox_results = dict(bbox_results)
        bbox_results.update(self.bbox_head.loss_and_target(cls, reg, rois, sampling_results, K))
        return bbox_results

    @torch.no_grad()
    def loss_and_grads(self, feats, rpn_results_list, batch_gt_instances, num_classes=None, fc_cls=None, fc_reg=None, generator=None, sample_inds=None,
                       return_samples=False):
        """one training pass without autograd -> (losses dict(loss_cls, loss_bbox, acc), {parameter name: gradient}, [d feats, NCHW f32]): the
        gradients of loss_cls + loss_bbox.  Parameter names: the bbox head's ('bbox_head.shared_fcs.0.weight', ...); predictors passed per call
        appear as 'fc_cls.*' / 'fc_reg.*'.  return_samples: a fourth value, the sampling results (their 'pos' feeds the mask half)."""
        h, ex = self.bbox_head, self.bbox_roi_extractor
        s = self.gen_sampling_results(rpn_results_list, batch_gt_instances, generator, sample_inds)
        rows, maps, sizes, images = self._levels(feats)
        valid = (s["n_pos"] + s["n_neg"]).contiguous()
        levels = torch.empty(s["rois"].shape[0], device=s["rois"].device, dtype=torch.int32)
        x = ex.extract(maps, sizes, images, s["rois"], valid=valid, levels_out=levels)
        R = x.shape[0]
        eng, out, c, K = h.forward_rows(x.view(R, -1), num_classes, fc_cls, fc_reg)
        dout = torch.zeros_like(out)      # the padding columns of the GEMM; the loss kernel stores every logit and every delta column itself
        losses = self._loss_rows(out, K, s, dout)
        _, fc, fr, names = h.predictors(num_classes, fc_cls, fc_reg)
        own = fc is getattr(h, "fc_cls", None)
        G = {n: torch.zeros_like(p) for n, p in h.named_parameters()}
        if not own:
            G.update({"fc_cls.weight": torch.zeros_like(fc.weight), "fc_cls.bias": torch.zeros_like(fc.bias), "fc_reg.weight": torch.zeros_like(fr.weight),
                      "fc_reg.bias": torch.zeros_like(fr.bias)})
        dx = h.backward_rows(eng, dout, c, G, names, K)
        grads = {("bbox_head." + n if (own or n.startswith("shared_fcs.")) else n): g for n, g in G.items()}
        drows = [torch.empty_like(r) for r in rows]      # the RoIAlign backward stores every pixel
        dmaps = [(d,) + m[1:] for d, m in zip(drows, maps)]
        ex.extract_bwd(dx.view(R, -1, ex.out_channels), dmaps, sizes, images, s["rois"], roi_levels=levels, valid=valid)
        dfeats = [DecodeEngine.to_nchw(d, images, H, W) for d, (H, W) in zip(drows, sizes)]
        return (losses, grads, dfeats, s) if return_samples else (losses, grads, dfeats)

    # ------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict_bbox(self, batch_img_metas, bbox_results, proposals, rois, rcnn_test_cfg=None, num_classes=None, rescale=False):
        """the reference's signature: bbox_results with cls_score (R, K + 1) and bbox_pred (R, 4 K) of rois (R, 5) -> per image an object with bboxes
        (k, 4), scores (k), labels (k) and .keep: what MaskRoIHead.predict takes.  rcnn_test_cfg None: the raw boxes and scores."""
        cls = bbox_results["cls_score"].detach().to(F32).contiguous()
        reg = bbox_results["bbox_pred"].detach().to(F32).contiguous()
        return self.bbox_head.predict_by_feat(rois, cls, reg, batch_img_metas, num_classes, rcnn_test_cfg, rescale, [int(p.shape[0]) for p in proposals])

    @torch.no_grad()
    def predict(self, x, rpn_results_list, batch_img_metas=None, rescale=False, num_classes=None, fc_cls=None, fc_reg=None, rcnn_test_cfg=None):
        """proposals in, detections out: test_bbox_generate_roi -> RoIAlign -> the layers -> predict_by_feat (test_cfg unless rcnn_test_cfg)"""
        h = self.bbox_head
        proposals, rois = self.test_bbox_generate_roi(rpn_results_list)
        K = h.predictors(num_classes, fc_cls, fc_reg)[0]
        cfg = self.test_cfg if rcnn_test_cfg is None else rcnn_test_cfg
        if batch_img_metas is None or len(batch_img_metas) != len(proposals):
            raise ValueError("%s: one img_meta with img_shape per image (the boxes are clipped to it)" % type(self).__name__)
        if rois.shape[0] == 0:
            return h.predict_by_feat(rois, None, None, batch_img_metas, K, cfg, rescale, [0] * len(proposals))
        _, maps, sizes, images = self._levels(x)
        feats = self.bbox_roi_extractor.extract(maps, sizes, images, rois)
        _, out, _, K = h.forward_rows(feats.view(feats.shape[0], -1), num_classes, fc_cls, fc_reg)
        c0 = h.reg_col(K)
        return h.predict_by_feat(rois, out[:, :K + 1], out[:, c0:c0 + 4 * K], batch_img_metas, K, cfg, rescale, [int(p.shape[0]) for p in proposals])
