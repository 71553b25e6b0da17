"""MTP_IS_StandardRoIHead: the mask half of the reference's instance-segmentation RoI head (instance_segmentation/roi_head.py: init_mask_head,
train_mask_forward, mask_loss, test_mask_generate_rois, test_mask_roi_feats, predict_mask; configured at mask_rcnn.py:56-68, 92-119):
SingleRoIExtractor (RoIAlign 14, adaptive grid) -> FCNMaskHead -> the data set's 1x1 conv_logits -> mask targets + binary cross-entropy, and the
paste at test time.  The horizontal box half (bbox_roi_extractor, bbox_head) is a class of its own, hbox_roi_head.HBoxRoIHead; asking this one for it raises.

Training takes the positives in either of two forms: the reference's list of per-image sampling results (pos_priors, pos_assigned_gt_inds,
pos_gt_labels), or the fixed-slot form of the oriented head -- S slots per image, the first n_pos[b] of them positives, n_pos on the device.  The
list is laid into the same slots (its lengths are shapes), so both forms run the same launches and give the same bits.  On the slot form nothing
between the samples and the loss synchronises with the host: one RoIAlign launch, the head's GEMMs, two loss launches, and back."""
import torch
import torch.nn as nn

from .. import ops
from ..engine_decode import DecodeEngine
from ..registry import MODELS
from ._cfg import field as _get, optional as _opt, strip_scope as _strip
from .mask_head import stack_bitmaps

F32 = torch.float32


@MODELS.register_module(name=["MTP_IS_StandardRoIHead"])
class MaskRoIHead(nn.Module):
    """MTP_IS_StandardRoIHead(mask_roi_extractor, mask_head, train_cfg, test_cfg).  conv_logits, the 1x1 Conv2d of the data set at hand, is passed per
    call; its number of output channels is the class count."""

    def __init__(self, bbox_roi_extractor=None, bbox_head=None, mask_roi_extractor=None, mask_head=None, shared_head=None, train_cfg=None, test_cfg=None,
                 init_cfg=None):
        super().__init__()
        me = "MTP_IS_StandardRoIHead"
        if bbox_roi_extractor is not None or bbox_head is not None:
            raise NotImplementedError("%s: the horizontal box half (bbox_roi_extractor, bbox_head) is not built; this class is the mask half" % me)
        if shared_head is not None:
            raise NotImplementedError("%s: a shared head is not built" % me)
        if mask_head is None:
            raise TypeError("%s: mask_head is needed" % me)
        if mask_roi_extractor is None:
            raise NotImplementedError("%s: share_roi_extractor (a mask head without its own mask_roi_extractor) is not built" % me)
        self.mask_roi_extractor = mask_roi_extractor if isinstance(mask_roi_extractor, nn.Module) else MODELS.build(_strip(mask_roi_extractor, "mmdet."))
        self.mask_head = mask_head if isinstance(mask_head, nn.Module) else MODELS.build(_strip(mask_head, "mmdet."))
        self.share_roi_extractor = False
        if self.mask_roi_extractor.out_channels != self.mask_head.in_channels or self.mask_roi_extractor.roi_layers[0].output_size != self.mask_head.roi_feat_size[0]:
            raise ValueError("%s: the extractor's output is the mask head's input" % me)
        self.train_cfg, self.test_cfg = (None if train_cfg is None else dict(train_cfg)), (None if test_cfg is None else dict(test_cfg))
        self.slots = None
        if self.train_cfg is not None:
            if self.train_cfg.get("soft_mask_target", False):
                raise NotImplementedError("%s: soft_mask_target=True is not built (no MTP configuration sets it)" % me)
            size = self.train_cfg.get("mask_size", self.mask_head.mask_size)
            size = size[0] if isinstance(size, (tuple, list)) else size
            if int(size) != self.mask_head.mask_size:
                raise ValueError("%s: mask_size %d is not the size of the mask head's output (%d)" % (me, size, self.mask_head.mask_size))
            sampler = self.train_cfg.get("sampler")
            if sampler is not None:      # the most positives an image can have: the slots the reference's lists are laid into
                self.slots = max(1, int(sampler.get("num", 512) * sampler.get("pos_fraction", 0.25)))

    with_bbox, with_mask, with_shared_head = False, True, False
    head_chunk = 1024      # slots the mask head's layers take at a time

    def init_mask_head(self, mask_roi_extractor, mask_head):
        raise RuntimeError("MTP_IS_StandardRoIHead: the mask head is built by the constructor")

    def invalidate_weights(self):
        """the parameters were written through raw pointers (see FCNMaskHead.invalidate_weights)"""
        self.mask_head.invalidate_weights()

    # ------------------------------------------------------------------ samples
    def as_slots(self, samples, gt_masks, device):
        """-> dict(boxes (images * S, 4), rois (images * S, 5), sample_gt (images, S) rows of bitmaps, labels (images * S), n_pos (images), bitmaps
        (G, H, W) uint8, img_hw (images, 2) or None).  samples: the slot form -- a dict with boxes (images * S, 4) or rois (images * S, 5),
        sample_gt (images, S), n_pos (images) and labels (images * S) or gt_labels (G) -- or the reference's list of sampling results.  gt_masks:
        see stack_bitmaps.  No host synchronisation."""
        bm, hw, start = stack_bitmaps(gt_masks, device)
        if isinstance(samples, dict):
            sample_gt = samples["sample_gt"].to(device=device, dtype=torch.int64).contiguous()
            images, S = sample_gt.shape
            boxes = samples["boxes"] if "boxes" in samples else samples["rois"][:, 1:]
            boxes = boxes.detach().to(device=device, dtype=F32).reshape(images * S, 4).contiguous()
            n_pos = samples["n_pos"].to(device=device, dtype=torch.int64).contiguous()
            if samples.get("labels") is not None:
                labels = samples["labels"].to(device=device, dtype=torch.int64).reshape(-1).contiguous()
            elif samples.get("gt_labels") is None:
                labels = sample_gt.new_zeros(images * S)
            else:      # the assigned gt's label; rows out of range are padding to the kernel whatever label they get
                gl = samples["gt_labels"].to(device=device, dtype=torch.int64)
                labels = gl[sample_gt.reshape(-1).clamp(0, max(gl.numel() - 1, 0))].contiguous() if gl.numel() else sample_gt.new_zeros(images * S)
        else:
            if start is None:
                raise ValueError("MTP_IS_StandardRoIHead: with a list of sampling results the bitmaps come per image")
            images = len(samples)
            counts = [int(_get(r, "pos_priors").shape[0]) for r in samples]      # shapes, not device values
            S = max([self.slots or 1] + counts)
            boxes = torch.zeros(images, S, 4, device=device, dtype=F32)
            sample_gt = torch.full((images, S), -1, device=device, dtype=torch.int64)
            labels = torch.zeros(images, S, device=device, dtype=torch.int64)
            for b, (r, n) in enumerate(zip(samples, counts)):
                boxes[b, :n] = _get(r, "pos_priors").detach().to(device=device, dtype=F32).reshape(-1, 4)
                sample_gt[b, :n] = _get(r, "pos_assigned_gt_inds").to(device=device, dtype=torch.int64).reshape(-1) + start[b]
                labels[b, :n] = _get(r, "pos_gt_labels").to(device=device, dtype=torch.int64).reshape(-1)
            boxes, labels = boxes.reshape(-1, 4), labels.reshape(-1)
            n_pos = torch.tensor(counts, device=device, dtype=torch.int64)
        image = torch.arange(images, device=device, dtype=F32).repeat_interleave(S)[:, None]
        return dict(boxes=boxes, rois=torch.cat([image, boxes], 1).contiguous(), sample_gt=sample_gt, labels=labels, n_pos=n_pos, bitmaps=bm, img_hw=hw,
                    images=images, S=S)

    # ------------------------------------------------------------------ RoI features
    def _levels(self, feats):
        """NCHW maps -> (buffers per level, triples, sizes, images, rows): (N H W, C) f32 rows, channel last, which is what the RoIAlign kernels
        read in whole lines; the layout kernels move four channels at a time, so a channel count that is no multiple of 4 stays NCHW (rows False)
        and is read through its strides"""
        ex = self.mask_roi_extractor
        feats = list(feats)[:ex.num_inputs]
        if len(feats) != ex.num_inputs or any(f.dim() != 4 or f.shape[1] != ex.out_channels for f in feats):
            raise ValueError("MTP_IS_StandardRoIHead: expected %d NCHW maps of %d channels" % (ex.num_inputs, ex.out_channels))
        sizes = [(int(f.shape[2]), int(f.shape[3])) for f in feats]
        if ex.out_channels % 4:
            bufs = [f.detach().to(F32).contiguous() for f in feats]
            return bufs, [ops.rpn_map_nchw(b) for b in bufs], sizes, int(feats[0].shape[0]), False
        eng = DecodeEngine(self, "fp32")
        bufs = [eng.to_rows(f.detach(), F32) for f in feats]
        return bufs, [ops.rpn_map_rows(r, H, W) for r, (H, W) in zip(bufs, sizes)], sizes, int(feats[0].shape[0]), True

    @staticmethod
    def bbox2roi(bbox_list):
        return torch.cat([torch.cat([b.new_full((b.shape[0], 1), float(i)), b.reshape(-1, 4)], 1) for i, b in enumerate(bbox_list)], 0) if len(bbox_list) \
            else torch.zeros(0, 5)

    @torch.no_grad()
    def train_mask_forward(self, x, sampling_results, bbox_feats=None):
        """the reference's signature -> mask_feats (positives, C, 14, 14) of the positives' boxes, image after image (bbox_feats is not used: the
        extractor is not shared).  A slot-form dict gives (images * S, C, 14, 14) with zeros on the padding."""
        if isinstance(sampling_results, dict):
            s = self.as_slots(sampling_results, dict(bitmaps=torch.zeros(0, 1, 1, dtype=torch.uint8)), x[0].device)
            _, maps, sizes, images, _ = self._levels(x)
            out = self.mask_roi_extractor.extract(maps, sizes, images, s["rois"], valid=s["n_pos"])
            P = self.mask_roi_extractor.roi_layers[0].output_size
            return out.permute(0, 2, 1).reshape(out.shape[0], -1, P, P)
        rois = self.bbox2roi([_get(r, "pos_priors").detach().to(F32) for r in sampling_results])
        return self.test_mask_roi_feats(x, rois)

    def test_mask_generate_rois(self, results_list):
        return self.bbox2roi([_get(r, "bboxes").detach().to(F32) for r in results_list]).contiguous()

    def test_mask_roi_feats(self, x, rois=None, pos_inds=None, bbox_feats=None):
        if rois is None or pos_inds is not None or bbox_feats is not None:
            raise NotImplementedError("MTP_IS_StandardRoIHead: share_roi_extractor (pos_inds, bbox_feats) is not built; pass rois")
        return self.mask_roi_extractor(list(x)[:self.mask_roi_extractor.num_inputs], rois)

    def _mask_forward(self, x, rois, conv_logits):
        mask_feats = self.test_mask_roi_feats(x, rois)
        return dict(mask_preds=self.mask_head(mask_feats, conv_logits), mask_feats=mask_feats)

    # ------------------------------------------------------------------ loss
    @torch.no_grad()
    def mask_loss(self, mask_results, sampling_results, batch_gt_instances):
        """the reference's signature: mask_results['mask_preds'] (positives, num_classes, 28, 28) of the sampled positives -> mask_results with
        loss_mask = dict(loss_mask=...)"""
        out = self.mask_head.loss_and_target(mask_results["mask_preds"], sampling_results, batch_gt_instances, self.train_cfg)
        mask_results = dict(mask_results)
        mask_results.update(loss_mask=out["loss_mask"], mask_targets=out["mask_targets"])
        return mask_results

    @torch.no_grad()
    def loss_and_grads(self, feats, samples, gt_masks, conv_logits, return_aux=False):
        """one training pass without autograd -> (dict(loss_mask), {parameter name: gradient}, [d feats, NCHW f32]): the gradients of loss_mask with
        respect to every level map, every parameter of the mask head ('mask_head.convs.0.conv.weight', ...) and conv_logits ('conv_logits.weight',
        'conv_logits.bias').  return_aux: a fourth value, dict(mask_feats (slots, 196, C), mask_preds (slots, K, 28, 28), mask_targets (slots, 28,
        28) uint8, slot_loss, levels), in slot order."""
        h, ex = self.mask_head, self.mask_roi_extractor
        dev = feats[0].device
        s = self.as_slots(samples, gt_masks, dev)
        bufs, maps, sizes, images, as_rows = self._levels(feats)
        if images != s["images"]:
            raise ValueError("MTP_IS_StandardRoIHead: %d images of samples for maps of %d images" % (s["images"], images))
        R, S = s["rois"].shape[0], ex.roi_layers[0].output_size
        levels = torch.empty(R, device=dev, dtype=torch.int32)
        x = ex.extract(maps, sizes, images, s["rois"], valid=s["n_pos"], levels_out=levels)
        # the head runs over at most head_chunk slots at a time (its GEMMs and layout kernels keep the sizes the decode heads run them at); the
        # loss sees the whole batch, because its mean is over the positives of all images
        parts, preds = [], None
        for r0 in range(0, R, self.head_chunk):
            r1 = min(R, r0 + self.head_chunk)
            eng, c, _, p, lc, K = h.forward_rows(x[r0:r1].view((r1 - r0) * S * S, -1), r1 - r0, S, conv_logits)
            if r1 - r0 == R:
                preds = p
            else:
                preds = torch.empty((R,) + tuple(p.shape[1:]), device=dev, dtype=F32) if preds is None else preds
                preds[r0:r1].copy_(p)
            parts.append((r0, r1, eng, c, lc))
        dl = torch.empty_like(preds)      # the loss kernel stores every element
        out = ops.mask_loss(preds, s["boxes"], None if h.class_agnostic else s["labels"], s["sample_gt"], s["n_pos"], s["bitmaps"], s["img_hw"], h.loss_weight,
                            dlogits=dl, num_classes=K)
        names = ("conv_logits.weight", "conv_logits.bias" if conv_logits.bias is not None else None)

        def zeros():
            g = {n: torch.zeros_like(p) for n, p in h.named_parameters()}
            g.update({n: torch.zeros_like(getattr(conv_logits, n.split(".")[1])) for n in names if n is not None})
            return g
        G, dx = zeros(), torch.empty_like(x)
        for i, (r0, r1, eng, c, lc) in enumerate(parts):      # chunk after chunk, added in that order
            Gc = G if i == 0 else zeros()
            dfeat = eng.logits_bwd_rows(eng.to_rows_like(dl[r0:r1], c), lc, Gc, names)
            dx[r0:r1].copy_(eng.head_bwd(dfeat, c, Gc).view(r1 - r0, S * S, -1))
            if i:
                for n in G:
                    G[n].add_(Gc[n])
        grads = {(n if n.startswith("conv_logits.") else "mask_head." + n): g for n, g in G.items()}
        dbufs = [torch.empty_like(r) for r in bufs]      # the RoIAlign backward stores every pixel
        dmaps = [(d,) + m[1:] for d, m in zip(dbufs, maps)]
        ex.extract_bwd(dx.view(R, S * S, ex.out_channels), dmaps, sizes, images, s["rois"], roi_levels=levels, valid=s["n_pos"])
        dfeats = [DecodeEngine.to_nchw(d, images, H, W) for d, (H, W) in zip(dbufs, sizes)] if as_rows else dbufs
        losses = dict(loss_mask=out["loss"][0])
        if return_aux:
            return losses, grads, dfeats, dict(mask_feats=x, mask_preds=preds[:, :K], mask_targets=out["targets"], slot_loss=out["slot_loss"], levels=levels)
        return losses, grads, dfeats

    def loss(self, x, samples, gt_masks, conv_logits):
        """-> dict(loss_mask), no gradients"""
        with torch.no_grad():
            h, ex = self.mask_head, self.mask_roi_extractor
            s = self.as_slots(samples, gt_masks, x[0].device)
            _, maps, sizes, images, _ = self._levels(x)
            R, S = s["rois"].shape[0], ex.roi_layers[0].output_size
            feats = ex.extract(maps, sizes, images, s["rois"], valid=s["n_pos"])
            preds = torch.cat([h.forward_rows(feats[r0:r0 + self.head_chunk].view(-1, feats.shape[2]), min(R, r0 + self.head_chunk) - r0, S, conv_logits)[3]
                               for r0 in range(0, R, self.head_chunk)]) if R > self.head_chunk else h.forward_rows(feats.view(R * S * S, -1), R, S, conv_logits)[3]
            out = ops.mask_loss(preds, s["boxes"], None if h.class_agnostic else s["labels"], s["sample_gt"], s["n_pos"], s["bitmaps"], s["img_hw"], h.loss_weight,
                                num_classes=int(conv_logits.weight.shape[0]))
            return dict(loss_mask=out["loss"][0])

    # ------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict_mask(self, batch_img_metas, results_list, mask_results, rescale=False):
        """the reference's signature: mask_results['mask_preds'] (all instances, num_classes, 28, 28), split per image by the lengths of
        results_list -> results_list with .masks"""
        counts = [int(_get(r, "bboxes").shape[0]) for r in results_list]
        preds = mask_results["mask_preds"].split(counts, 0)
        return self.mask_head.predict_by_feat(preds, results_list, batch_img_metas, self.test_cfg, rescale=rescale)

    def predict(self, x, results_list, batch_img_metas, conv_logits, rescale=False):
        """boxes in, masks out: test_mask_generate_rois -> test_mask_roi_feats -> mask_head + conv_logits -> predict_mask"""
        rois = self.test_mask_generate_rois(results_list).to(x[0].device)
        return self.predict_mask(batch_img_metas, results_list, self._mask_forward(x, rois, conv_logits), rescale)
