"""HBoxShared2FCBBoxHead: the reference's MTP_IS_Shared2FCBBoxHead (instance_segmentation/bbox_head.py, base_bbox_head.py; configured at
mask_rcnn.py:37-55), the bbox head of Mask R-CNN: two shared fully connected layers with ReLU, a softmax fc_cls and a PER-CLASS fc_reg (4 K
deltas per RoI; the loss picks the four of the label, the prediction decodes K boxes per RoI), DeltaXYWHBBoxCoder, L1.

Two forms, as Shared2FCBBoxHead has them: with num_classes the head owns fc_cls (K + 1) / fc_reg (4 K); without (the reference's form,
models.py:156-166, 253-281) forward returns (x_cls, x_reg) and num_classes, fc_cls, fc_reg of the data set at hand come per call.

reg_target.  base_bbox_head.py:430-435 calls self.loss_bbox(pos_bbox_pred, bbox_weights[pos], avg_factor=...): the target argument is commented
out and the all-ones weights stand in its place, so the reference regresses the label's four deltas towards 1.  'reference' (the default of the
class registered under the reference's name) reproduces that; 'encoded' is mmdet's behaviour, L1 against coder.encode(roi, gt).  The kernel has
both.

The layers run on engine_roi.  The K + 1 logits are padded with zero rows to a multiple of 4 columns there, so that every class's four deltas are
one 16-byte access of mtp_amd.ops.hroi_loss / hroi_predict."""
from types import SimpleNamespace

import torch

from .. import ops
from ..registry import MODELS
from .bbox_head import Shared2FCBBoxHead

F32 = torch.float32
NAMES = ("fc_cls.weight", "fc_cls.bias", "fc_reg.weight", "fc_reg.bias")


@MODELS.register_module(name=["MTP_IS_Shared2FCBBoxHead"])
class HBoxShared2FCBBoxHead(Shared2FCBBoxHead):
    """State dict: shared_fcs.{0,1}.{weight,bias}, and with num_classes fc_cls.* (num_classes + 1 rows) and fc_reg.* (4 * num_classes rows)."""

    DELTAS, BOX_TYPE, CODER_SCOPE, CODER_NAME = ops.HBOX_DELTAS, "hbox", "mmdet.", "the delta-xywh coder (four deltas)"

    def __init__(self, in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=None, num_shared_convs=0, num_shared_fcs=2, with_avg_pool=False,
                 with_cls=True, with_reg=True, predict_box_type="hbox", reg_class_agnostic=False, reg_decoded_bbox=False,
                 reg_predictor_cfg=dict(type="mmdet.Linear"), cls_predictor_cfg=dict(type="mmdet.Linear"),
                 bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2)),
                 loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
                 reg_target="reference", precision="fp32", init_cfg=None):
        if reg_target not in ops.HROI_TARGET:
            raise ValueError("%s: reg_target is 'reference' (base_bbox_head.py as written: the target is 1) or 'encoded' (mmdet), got %r"
                             % (type(self).__name__, reg_target))
        super().__init__(in_channels, fc_out_channels, roi_feat_size, num_classes, num_shared_convs, num_shared_fcs, with_avg_pool, with_cls, with_reg,
                         predict_box_type, reg_class_agnostic, reg_decoded_bbox, reg_predictor_cfg, cls_predictor_cfg, bbox_coder, loss_cls, loss_bbox, precision,
                         init_cfg)
        self.reg_target = reg_target

    def _check_regression(self, reg_class_agnostic, lb, loss_bbox):
        me = type(self).__name__
        if reg_class_agnostic:
            raise NotImplementedError("%s: reg_class_agnostic=True is not built (mask_rcnn.py regresses one box per class)" % me)
        if lb["type"] != "L1Loss":
            raise NotImplementedError("%s: loss_bbox %r is not built (L1Loss is what mask_rcnn.py configures)" % (me, loss_bbox))

    def reg_width(self, num_classes):
        return self.DELTAS * num_classes

    # ------------------------------------------------------------------ the layers
    def predictors(self, num_classes=None, fc_cls=None, fc_reg=None):
        """-> (num_classes, fc_cls, fc_reg, names of their gradients): the head's own, or the ones passed (both, with num_classes)"""
        if fc_cls is None and fc_reg is None and self.num_classes is not None and num_classes in (None, self.num_classes):
            return self.num_classes, self.fc_cls, self.fc_reg, NAMES
        me = type(self).__name__
        if fc_cls is None or fc_reg is None or num_classes is None:
            raise ValueError("%s: without its own num_classes the head takes num_classes, fc_cls and fc_reg per call" % me)
        if tuple(fc_cls.weight.shape) != (num_classes + 1, self.cls_last_dim) or tuple(fc_reg.weight.shape) != (4 * num_classes, self.reg_last_dim):
            raise ValueError("%s: fc_cls is Linear(%d, num_classes + 1) and fc_reg Linear(%d, 4 * num_classes)" % (me, self.cls_last_dim, self.reg_last_dim))
        if fc_cls.bias is None or fc_reg.bias is None:
            raise NotImplementedError("%s: fc_cls and fc_reg have a bias" % me)
        return int(num_classes), fc_cls, fc_reg, NAMES

    @staticmethod
    def reg_col(K):
        """the column of the first delta in the rows of forward_rows: K + 1 logits rounded up to a multiple of 4"""
        return -(-(K + 1) // 4) * 4

    def forward_rows(self, rows, num_classes=None, fc_cls=None, fc_reg=None):
        """rows (R, bins * C) f32 in (bin, c) order -> (engine, out (R, Kp) f32, context, K): logits in columns 0 .. K, class k's deltas in
        reg_col(K) + 4 k .. + 4"""
        K, fc, fr, _ = self.predictors(num_classes, fc_cls, fc_reg)
        pad = self.reg_col(K) - (K + 1)
        w, b = fc.weight.detach(), fc.bias.detach()
        if pad:      # zero rows: their logits are 0 and nothing reads them
            w, b = torch.cat([w, w.new_zeros(pad, w.shape[1])]), torch.cat([b, b.new_zeros(pad)])
        eng = self.engine()
        out, c = eng.forward_rows(rows, self.roi_feat_area, self._shared(), w, b, fr.weight, fr.bias)
        return eng, out, c, K

    def backward_rows(self, eng, dout, c, G, names, K):
        """engine_roi's backward with the padded logits: G[fc_cls.*] get the first K + 1 rows of what the engine computes"""
        if self.reg_col(K) == K + 1:
            return eng.backward_rows(dout, c, G, names)
        wide = dict(G)
        wide[names[0]] = G[names[0]].new_zeros(self.reg_col(K), G[names[0]].shape[1])
        wide[names[1]] = G[names[1]].new_zeros(self.reg_col(K))
        dx = eng.backward_rows(dout, c, wide, names)
        G[names[0]].copy_(wide[names[0]][:K + 1])
        G[names[1]].copy_(wide[names[1]][:K + 1])
        return dx

    @torch.no_grad()
    def forward(self, x, num_classes=None, fc_cls=None, fc_reg=None):
        """x (R, C, 7, 7).  With predictors (the head's own or passed) -> (cls_score (R, K + 1), bbox_pred (R, 4 K)) f32; without -> (x_cls, x_reg),
        the output of the shared layers, f32.  No autograd graph: training goes through HBoxRoIHead.loss_and_grads."""
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.in_channels, self.roi_feat_size, self.roi_feat_size):
            raise ValueError("%s: expected (R, %d, %d, %d) RoI features" % (type(self).__name__, self.in_channels, self.roi_feat_size, self.roi_feat_size))
        R = x.shape[0]
        own = self.num_classes is not None or fc_cls is not None
        if R == 0:
            if own:
                K = self.predictors(num_classes, fc_cls, fc_reg)[0]
                return x.new_zeros((0, K + 1), dtype=F32), x.new_zeros((0, 4 * K), dtype=F32)
            e = x.new_zeros((0, self.fc_out_channels), dtype=F32)
            return e, e
        rows = self.rows_of(x)
        if not own:
            y = self.engine().shared_rows(rows, self.roi_feat_area, self._shared()).to(F32)
            return y, y
        _, out, _, K = self.forward_rows(rows, num_classes, fc_cls, fc_reg)
        c0 = self.reg_col(K)
        return out[:, :K + 1].contiguous(), out[:, c0:c0 + 4 * K].contiguous()

    # ------------------------------------------------------------------ loss
    @torch.no_grad()
    def loss_and_target(self, cls_score, bbox_pred, rois, sampling_results, num_classes=None, dcls=None, dreg=None, **kwargs):
        """cls_score (images * num, K + 1), bbox_pred (images * num, 4 K) rows (column slices of a wider buffer are fine), rois (images * num, 5),
        sampling_results: the slot dict of HBoxRoIHead.gen_sampling_results -> dict(loss_bbox=dict(loss_cls, loss_bbox, acc)); dcls / dreg: buffers
        for the gradients in the layout of their inputs"""
        K = self.num_classes if num_classes is None else int(num_classes)
        s = sampling_results
        l = ops.hroi_loss(cls_score, bbox_pred, K, rois[:, 1:].contiguous(), s["gts"], s["gt_labels"], s["sample_gt"], s["n_pos"], s["n_neg"],
                          self.bbox_coder.means, self.bbox_coder.stds, self.reg_target, self.cls_weight, self.bbox_weight, dcls, dreg)
        return dict(loss_bbox=dict(loss_cls=l[0], loss_bbox=l[1], acc=l[2]))

    # ------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict_by_feat(self, rois, cls_scores, bbox_preds, batch_img_metas, num_classes=None, rcnn_test_cfg=None, rescale=False, counts=None):
        """rois (R, 5) of the whole batch, image after image; cls_scores (R, K + 1), bbox_preds (R, 4 K) -> per image an object with bboxes (k, 4),
        scores (k), labels (k), descending score, and .keep (k): the (roi, class) candidates kept, as roi * K + class with roi counted inside the
        image.  counts: the RoIs of every image (HBoxRoIHead passes the lengths of the proposal lists, which are shapes); without them they are
        counted on the device, one more synchronisation, and every RoI must name an image below len(batch_img_metas).  rcnn_test_cfg None: the
        raw bboxes (n, 4 K) and scores (n, K + 1) per image; the kernel writes the K class scores, and the background column is 1 minus their
        sum (clamped at 0), which equals the softmax's own column but for the rounding of that sum.  One launch for the batch, then per image mmdet's
        multiclass_nms: the candidates above score_thr, NMS with the class as the group, max_per_img.  Host synchronisations: one per batch, for the
        numbers of candidates, and one per image, for the number NMS kept.  At most 32 768 candidates per image (more raise)."""
        K = self.num_classes if num_classes is None else int(num_classes)
        images, dev = len(batch_img_metas), rois.device
        if counts is None:
            counts = [0] * images if rois.shape[0] == 0 else torch.bincount(rois[:, 0].to(torch.int64), minlength=images)[:images].tolist()
        counts = [int(n) for n in counts]
        if len(counts) != images or sum(counts) != rois.shape[0]:
            raise ValueError("%s: one img_meta per image, and every RoI in one of them" % type(self).__name__)
        bounds = [0]
        for n in counts:
            bounds.append(bounds[-1] + n)
        cfg = None if rcnn_test_cfg is None else dict(rcnn_test_cfg)
        empty = lambda: SimpleNamespace(bboxes=torch.zeros(0, 4, device=dev), scores=torch.zeros(0, device=dev),      # noqa: E731
                                        labels=torch.zeros(0, dtype=torch.int64, device=dev), keep=torch.zeros(0, dtype=torch.int64, device=dev))
        if rois.shape[0] == 0:
            if cfg is None:
                return [SimpleNamespace(bboxes=torch.zeros(0, 4 * K, device=dev), scores=torch.zeros(0, K + 1, device=dev)) for _ in range(images)]
            return [empty() for _ in range(images)]
        shapes = self.bbox_coder.shape_table([tuple(m["img_shape"])[:2] for m in batch_img_metas], dev)
        inv = None
        if rescale:      # mmdet: bboxes * (1 / scale_factor) repeated twice; the reciprocal is taken in double and rounded once
            inv = self.bbox_coder.shape_table([(1.0 / float(m["scale_factor"][0]), 1.0 / float(m["scale_factor"][1])) for m in batch_img_metas], dev)
        score_thr = 0.0 if cfg is None else float(cfg.get("score_thr", 0.0))
        scores, boxes, flags = ops.hroi_predict(cls_scores, bbox_preds, K, rois.detach().to(F32).contiguous(), self.bbox_coder.means, self.bbox_coder.stds,
                                                shapes, inv, score_thr)
        if cfg is None:
            bg = (1.0 - scores.sum(1, keepdim=True)).clamp_(min=0.0)
            full = torch.cat([scores, bg], 1)
            return [SimpleNamespace(bboxes=boxes[a:b].reshape(b - a, 4 * K), scores=full[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
        max_per_img, nms_cfg = int(cfg.get("max_per_img", -1)), dict(cfg["nms"])
        if nms_cfg.pop("type", "nms") != "nms":
            raise NotImplementedError("%s: the detections go through 'nms'" % type(self).__name__)
        thr = float(nms_cfg["iou_threshold"])
        ok = flags.bool()
        masked = torch.where(ok, scores, scores.new_full((), -1.0))
        n_cand = torch.stack([ok[a:b].sum() for a, b in zip(bounds[:-1], bounds[1:])]).tolist()      # the synchronisation of the batch
        flat = boxes.view(-1, 4)
        results = []
        for (a, b), n in zip(zip(bounds[:-1], bounds[1:]), n_cand):
            if n == 0:
                results.append(empty())
                continue
            ops.check_nms_count(n)
            sc = scores[a:b].reshape(-1)
            cand = torch.sort(masked[a:b].reshape(-1), descending=True, stable=True)[1][:n]      # roi * K + class, roi counted inside the image
            kept, count = ops.nms_sorted(flat[a * K + cand].contiguous(), thr, (cand % K).contiguous(), False, max_per_img)
            sel = cand[kept[:int(count)]]      # the synchronisation of this image
            results.append(SimpleNamespace(bboxes=flat[a * K + sel], scores=sc[sel], labels=sel % K, keep=sel))
        return results
