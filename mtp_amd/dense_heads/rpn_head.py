"""RPNHead: the reference's MTP_IS_RPNHead (instance_segmentation/rpn_head.py over mmdet's AnchorHead; configured at mask_rcnn.py:19-34, 70-91,
110-114), the horizontal RPN of Mask R-CNN.

It is the oriented head with four deltas per anchor (DeltaXYWHBBoxCoder), L1 in place of SmoothL1, gts (K, 4) and proposals clipped to the image
inside the decode: the convolutions (engine_rpn), the anchors, the assigner, the sampler and the NMS are those of OrientedRPNHead; targets and
losses are mtp_amd.ops.hrpn_loss and the proposals of all images and levels mtp_amd.ops.hrpn_proposals (csrc/hbox_head.hip)."""
from .. import ops
from ..registry import MODELS
from .oriented_rpn_head import OrientedRPNHead, _type


@MODELS.register_module(name=["RPNHead", "MTP_IS_RPNHead", "mmdet.RPNHead"])
class RPNHead(OrientedRPNHead):
    """RPNHead(in_channels, feat_channels=256, num_convs=1, anchor_generator, bbox_coder, loss_cls, loss_bbox, train_cfg, test_cfg,
    precision='fp32').  State dict: rpn_conv / rpn_cls / rpn_reg .weight / .bias (rpn_reg: 4 A channels).  gt_instances carry .bboxes (K, 4) and
    .labels; the proposals are .bboxes (n, 4) x1 y1 x2 y2 inside the image's img_shape."""

    DELTAS, BOX_DIM, CODER_SCOPES, CODER_NAME = ops.HBOX_DELTAS, 4, ("mmdet.",), "the delta-xywh coder (four deltas)"

    def __init__(self, in_channels, feat_channels=256, num_convs=1, num_classes=1,
                 anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[0.0] * 4, target_stds=[1.0] * 4),
                 loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
                 reg_decoded_bbox=False, train_cfg=None, test_cfg=None, precision="fp32", init_cfg=None):
        super().__init__(in_channels, feat_channels, num_convs, num_classes, anchor_generator, bbox_coder, loss_cls, loss_bbox, reg_decoded_bbox, train_cfg,
                         test_cfg, precision, init_cfg)

    def _check_loss_bbox(self, loss_bbox):
        if _type(loss_bbox, "mmdet.") != "L1Loss":
            raise NotImplementedError("%s: loss_bbox %r is not built (L1Loss is what mask_rcnn.py configures)" % (type(self).__name__, loss_bbox))

    def _loss_op(self, cls, reg, sizes, flat, gts, samples, sample_gt, n_pos, n_neg, dcls, dreg):
        return ops.hrpn_loss(cls, reg, sizes, self.num_base_priors, flat, gts, samples, sample_gt, n_pos, n_neg, self.bbox_coder.means, self.bbox_coder.stds,
                             self.cls_weight, self.bbox_weight, dcls, dreg)

    def _proposals_op(self, cls, reg, sizes, flat, keep, counts, min_size, images, batch_img_metas, device):
        if batch_img_metas is None or len(batch_img_metas) != images:
            raise ValueError("%s: one img_meta with img_shape per image (the proposals are clipped to it)" % type(self).__name__)
        shapes = self.bbox_coder.shape_table([tuple(m["img_shape"])[:2] for m in batch_img_metas], device)
        scores, boxes, level_ids, valid = ops.hrpn_proposals(cls, reg, sizes, self.num_base_priors, flat, keep, counts, self.bbox_coder.means,
                                                             self.bbox_coder.stds, shapes, min_size)
        return scores, boxes, boxes, level_ids, valid


MTP_IS_RPNHead = RPNHead
