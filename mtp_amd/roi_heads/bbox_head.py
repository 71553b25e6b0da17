"""Shared2FCBBoxHead: the reference's MTP_RD_Shared2FCBBoxHead (rotated_detection/bbox_head.py, base_bbox_head.py; configured at
oriented_rcnn.py:52-75): two shared fully connected layers with ReLU, then a class-agnostic fc_reg and a softmax fc_cls.

Two forms.  With num_classes the head owns fc_cls / fc_reg under mmdet's names (fine-tuning).  Without it (pretraining, models.py:224-251) the
head ends at the shared layers: forward returns (x_cls, x_reg), and num_classes, fc_cls and fc_reg of the data set at hand are passed per call.
The layers run on engine_roi; targets and losses are mtp_amd.ops.roi_loss, the per-RoI prediction is mtp_amd.ops.roi_predict."""
import torch
import torch.nn as nn

from .. import ops
from ..engine_roi import RoIFCEngine
from ..registry import MODELS, TASK_UTILS
from ._cfg import strip_scope as _strip

F32 = torch.float32


@MODELS.register_module(name=["Shared2FCBBoxHead", "MTP_RD_Shared2FCBBoxHead"])
class Shared2FCBBoxHead(nn.Module):
    """State dict: shared_fcs.{0,1}.{weight,bias}, and with num_classes fc_cls.* (num_classes + 1 rows) and fc_reg.* (5 rows)."""

    # what the per-class horizontal head (hbox_head.HBoxShared2FCBBoxHead) has otherwise, beside _check_regression and reg_width
    DELTAS, BOX_TYPE, CODER_SCOPE, CODER_NAME = ops.ROI_DELTAS, "rbox", "mmrotate.", "the delta-xywht coder (five deltas)"

    def __init__(self, in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=None, num_shared_convs=0, num_shared_fcs=2, with_avg_pool=False,
                 with_cls=True, with_reg=True, predict_box_type="rbox", reg_class_agnostic=True, reg_decoded_bbox=False,
                 reg_predictor_cfg=dict(type="mmdet.Linear"), cls_predictor_cfg=dict(type="mmdet.Linear"),
                 bbox_coder=dict(type="mmrotate.DeltaXYWHTRBBoxCoder", angle_version="le90", norm_factor=None, edge_swap=True, proj_xy=True,
                                 target_means=(.0, .0, .0, .0, .0), target_stds=(0.1, 0.1, 0.2, 0.2, 0.1)),
                 loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                 loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=1.0, loss_weight=1.0), precision="fp32", init_cfg=None):
        super().__init__()
        me = type(self).__name__
        if num_shared_convs > 0 or num_shared_fcs != 2:
            raise NotImplementedError("%s: two shared fully connected layers and no shared convolutions are what is built" % me)
        if with_avg_pool or not with_cls or not with_reg:
            raise NotImplementedError("%s: with_avg_pool, with_cls=False and with_reg=False are not built" % me)
        if reg_decoded_bbox:
            raise NotImplementedError("%s: reg_decoded_bbox is not built" % me)
        if predict_box_type != self.BOX_TYPE:
            raise NotImplementedError("%s: predict_box_type %r is not built" % (me, predict_box_type))
        for cfg in (reg_predictor_cfg, cls_predictor_cfg):
            if _strip(cfg, "mmdet.")["type"] != "Linear":
                raise NotImplementedError("%s: predictor %r is not built (Linear is)" % (me, cfg))
        lc, lb = _strip(loss_cls, "mmdet."), _strip(loss_bbox, "mmdet.")
        if lc["type"] != "CrossEntropyLoss" or lc.get("use_sigmoid", False) or lc.get("use_mask", False) or lc.get("class_weight") is not None:
            raise NotImplementedError("%s: loss_cls %r is not built (softmax CrossEntropyLoss, no class weights)" % (me, loss_cls))
        self._check_regression(reg_class_agnostic, lb, loss_bbox)
        if lc.get("reduction", "mean") != "mean" or lb.get("reduction", "mean") != "mean":
            raise NotImplementedError("%s: reduction other than 'mean' is not built" % me)
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        if in_channels % 8 or fc_out_channels % 8:
            raise ValueError("%s: in_channels and fc_out_channels must be multiples of 8 (the GEMM operands' rows are 16-byte chunks)" % me)
        self.in_channels, self.fc_out_channels, self.roi_feat_size, self.precision = int(in_channels), int(fc_out_channels), int(roi_feat_size), precision
        self.roi_feat_area = self.roi_feat_size ** 2
        self.reg_class_agnostic, self.reg_decoded_bbox, self.predict_box_type = bool(reg_class_agnostic), False, self.BOX_TYPE
        self.bbox_coder = TASK_UTILS.build(_strip(bbox_coder, self.CODER_SCOPE))
        if getattr(self.bbox_coder, "encode_size", None) != self.DELTAS:
            raise NotImplementedError("%s: the kernels are those of %s" % (me, self.CODER_NAME))
        self.cls_weight, self.bbox_weight, self.beta = float(lc.get("loss_weight", 1.0)), float(lb.get("loss_weight", 1.0)), float(lb.get("beta", 1.0))
        self.shared_fcs = nn.ModuleList([nn.Linear(self.in_channels * self.roi_feat_area, self.fc_out_channels),
                                         nn.Linear(self.fc_out_channels, self.fc_out_channels)])
        for m in self.shared_fcs:      # mmdet's init_cfg: Xavier uniform on the shared layers
            nn.init.xavier_uniform_(m.weight)
            nn.init.constant_(m.bias, 0.0)
        self.cls_last_dim = self.reg_last_dim = self.fc_out_channels
        self.num_classes = None if num_classes is None else int(num_classes)
        if self.num_classes is not None:
            if self.num_classes < 1:
                raise ValueError("%s: num_classes >= 1" % me)
            self.fc_cls = nn.Linear(self.cls_last_dim, self.num_classes + 1)
            self.fc_reg = nn.Linear(self.reg_last_dim, self.reg_width(self.num_classes))
            nn.init.normal_(self.fc_cls.weight, 0.0, 0.01)      # mmdet's init_cfg: Normal, std 0.01 / 0.001
            nn.init.normal_(self.fc_reg.weight, 0.0, 0.001)
            nn.init.constant_(self.fc_cls.bias, 0.0)
            nn.init.constant_(self.fc_reg.bias, 0.0)
        self._images = {}

    def _check_regression(self, reg_class_agnostic, lb, loss_bbox):
        me = type(self).__name__
        if not reg_class_agnostic:
            raise NotImplementedError("%s: reg_class_agnostic=False is not built (the MTP configurations regress one box per RoI)" % me)
        if lb["type"] != "SmoothL1Loss" or not lb.get("beta", 1.0) > 0:
            raise NotImplementedError("%s: loss_bbox %r is not built (SmoothL1Loss, beta > 0)" % (me, loss_bbox))

    def reg_width(self, num_classes):
        """the rows of fc_reg"""
        return self.DELTAS

    # ------------------------------------------------------------------ the layers
    def invalidate_weights(self):
        """shared_fcs.0.weight changed under torch's version counter (an optimizer kernel, a broadcast or any other write through the raw
        pointer): the next run permutes and packs its GEMM image again.  Writes through torch (load_state_dict, copy_, optimizer.step of
        torch.optim) are seen without this call; the images of the other layers are packed on every run."""
        self._images.clear()

    def engine(self):
        return RoIFCEngine(self, self.precision, self._images)

    def _shared(self):
        return {n: p for n, p in self.named_parameters() if n.startswith("shared_fcs.")}

    def predictors(self, num_classes=None, fc_cls=None, fc_reg=None):
        """-> (num_classes, fc_cls, fc_reg, names of their gradients): the head's own, or the ones passed (both, with num_classes)"""
        if fc_cls is None and fc_reg is None and self.num_classes is not None and num_classes in (None, self.num_classes):
            return self.num_classes, self.fc_cls, self.fc_reg, ("fc_cls.weight", "fc_cls.bias", "fc_reg.weight", "fc_reg.bias")
        if fc_cls is None or fc_reg is None or num_classes is None:
            raise ValueError("%s: without its own num_classes the head takes num_classes, fc_cls and fc_reg per call" % type(self).__name__)
        if tuple(fc_cls.weight.shape) != (num_classes + 1, self.cls_last_dim) or tuple(fc_reg.weight.shape) != (ops.ROI_DELTAS, self.reg_last_dim):
            raise ValueError("%s: fc_cls is Linear(%d, num_classes + 1) and fc_reg Linear(%d, 5)" % (type(self).__name__, self.cls_last_dim, self.reg_last_dim))
        if fc_cls.bias is None or fc_reg.bias is None:
            raise NotImplementedError("%s: fc_cls and fc_reg have a bias" % type(self).__name__)
        return int(num_classes), fc_cls, fc_reg, ("fc_cls.weight", "fc_cls.bias", "fc_reg.weight", "fc_reg.bias")

    def rows_of(self, x):
        """(R, C, h, w) RoI features in mmcv's layout -> (R, h * w * C) rows in the kernels' (bin, c) order"""
        R = x.shape[0]
        return x.detach().to(F32).reshape(R, self.in_channels, self.roi_feat_area).permute(0, 2, 1).reshape(R, -1).contiguous()

    def forward_rows(self, rows, num_classes=None, fc_cls=None, fc_reg=None):
        """rows (R, bins * C) f32 in (bin, c) order -> (engine, out (R, Kp) f32, context, K): logits in columns 0 .. K, deltas in K + 1 .. K + 5"""
        K, fc, fr, _ = self.predictors(num_classes, fc_cls, fc_reg)
        eng = self.engine()
        out, c = eng.forward_rows(rows, self.roi_feat_area, self._shared(), fc.weight, fc.bias, fr.weight, fr.bias)
        return eng, out, c, K

    @torch.no_grad()
    def forward(self, x, num_classes=None, fc_cls=None, fc_reg=None):
        """x (R, C, 7, 7).  With predictors (the head's own or passed) -> (cls_score (R, K + 1), bbox_pred (R, 5)) f32; without -> (x_cls, x_reg), the
        output of the shared layers, f32.  No autograd graph: training goes through StandardRoIHead.loss_and_grads."""
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.in_channels, self.roi_feat_size, self.roi_feat_size):
            raise ValueError("%s: expected (R, %d, %d, %d) RoI features" % (type(self).__name__, self.in_channels, self.roi_feat_size, self.roi_feat_size))
        R = x.shape[0]
        own = self.num_classes is not None or fc_cls is not None
        if R == 0:
            if own:
                K = self.predictors(num_classes, fc_cls, fc_reg)[0]
                return x.new_zeros((0, K + 1), dtype=F32), x.new_zeros((0, ops.ROI_DELTAS), dtype=F32)
            e = x.new_zeros((0, self.fc_out_channels), dtype=F32)
            return e, e
        rows = self.rows_of(x)
        if not own:
            y = self.engine().shared_rows(rows, self.roi_feat_area, self._shared()).to(F32)
            return y, y
        _, out, _, K = self.forward_rows(rows, num_classes, fc_cls, fc_reg)
        return out[:, :K + 1].contiguous(), out[:, K + 1:K + 1 + ops.ROI_DELTAS].contiguous()
