"""EncoderDecoder (mmseg EncoderDecoder as the reference carries it: Multi-Task_Pretrain/semantic_segmentation/encoder_decoder.py, and every
segmentation fine-tune config's `test_cfg=dict(mode='slide', stride=(384, 384), crop_size=(512, 512))`): backbone + decode head with whole-image and
sliding-window inference on the kernels of csrc/seg_eval.hip.

The head's logits stay channels-last rows from the classifier GEMM to the arg-max: each window's low-resolution logits are resized and added into an
f32 accumulator (N, H, W, Kp) in one launch, and one pass over the accumulator divides by the window count, takes the arg-max and -- with an IoUMetric
and labels -- counts the areas.  The window count is a grid product, so it travels as two small vectors cy (H) and cx (W).
"""
import torch
import torch.nn as nn

from .. import ops
from ..registry import MODELS

F32 = torch.float32


def slide_origins(size, crop, stride):
    """window origins along one axis (encoder_decoder.py:274-289): a grid of `stride`, the last window clamped back to max(end - crop, 0)"""
    grids = max(size - crop + stride - 1, 0) // stride + 1
    return [max(min(i * stride + crop, size) - crop, 0) for i in range(grids)]


def window_counts(size, crop, stride):
    """(size,) int32: how many windows of one axis cover each position; count_mat[y, x] = window_counts(H)[y] * window_counts(W)[x]"""
    c = torch.zeros(size, dtype=torch.int32)
    for a in slide_origins(size, crop, stride):
        c[a:a + crop] += 1
    return c


def _cfg(cfg, key, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


@MODELS.register_module()
class EncoderDecoder(nn.Module):
    """EncoderDecoder(backbone, decode_head, test_cfg=None, neck=None, auxiliary_head=None, ...): backbone and decode_head are modules or config dicts
    (built through MODELS).  test_cfg: dict(mode='whole') or dict(mode='slide', crop_size=(h, w), stride=(h, w))."""

    def __init__(self, backbone, decode_head, test_cfg=None, neck=None, auxiliary_head=None, train_cfg=None, data_preprocessor=None, pretrained=None,
                 init_cfg=None):
        super().__init__()
        if neck is not None or auxiliary_head is not None:
            raise NotImplementedError("EncoderDecoder: neck / auxiliary_head are not implemented (no MTP segmentation config sets them)")
        self.backbone = MODELS.build(backbone) if isinstance(backbone, dict) else backbone
        self.decode_head = MODELS.build(decode_head) if isinstance(decode_head, dict) else decode_head
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.out_channels = self.decode_head.out_channels
        if self.out_channels > ops.SEG_MAX_CLASSES:
            raise ValueError("EncoderDecoder: at most %d classes (got %d)" % (ops.SEG_MAX_CLASSES, self.out_channels))
        mode = _cfg(test_cfg, "mode", "whole")
        if mode not in ("slide", "whole"):
            raise ValueError("test_cfg.mode must be 'slide' or 'whole', got %r" % (mode,))
        if mode == "slide" and (_cfg(test_cfg, "crop_size") is None or _cfg(test_cfg, "stride") is None):
            raise ValueError("test_cfg mode='slide' needs crop_size and stride")
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    # ------------------------------------------------------------------ reference surface
    def extract_feat(self, inputs):
        return self.backbone(inputs)

    def encode_decode(self, inputs):
        """-> (logits (N*h*w, Kp) f32 rows on the head's output grid, columns K .. Kp zero; (N, h, w)): the head's eval-mode schedule, no NCHW round trip"""
        return self.decode_head.logit_rows(self.extract_feat(inputs))

    def whole_inference(self, inputs):
        """-> (acc (N, H, W, Kp) f32: the logits resized to the image, None, None)"""
        logits, (N, h, w) = self.encode_decode(inputs)
        H, W = int(inputs.shape[2]), int(inputs.shape[3])
        acc = ops._scratch((N, H, W, logits.shape[1]), logits.device, F32)
        ops.resize_bilinear_fwd(logits, acc.view(N * H * W, -1), N, h, w, H, W)
        return acc, None, None

    def slide_inference(self, inputs):
        """-> (acc (N, H, W, Kp) f32: the SUM of the windows' logits, cy (H) int32, cx (W) int32); seg_logits = acc / (cy[:, None] * cx[None, :])"""
        hs, ws = _pair(_cfg(self.test_cfg, "stride"))
        hc, wc = _pair(_cfg(self.test_cfg, "crop_size"))
        N, _, H, W = (int(s) for s in inputs.shape)
        if H < hc or W < wc:
            raise ValueError("slide_inference: the %d x %d image is smaller than the %d x %d crop (the backbone's pos_embed is fixed: pad the image)"
                             % (H, W, hc, wc))
        cy, cx = window_counts(H, hc, hs), window_counts(W, wc, ws)
        if int(cy.min()) == 0 or int(cx.min()) == 0:
            raise ValueError("slide_inference: stride %s larger than crop %s leaves pixels that no window covers" % ((hs, ws), (hc, wc)))
        acc = None
        for y1 in slide_origins(H, hc, hs):
            for x1 in slide_origins(W, wc, ws):
                logits, (_, h, w) = self.encode_decode(inputs[:, :, y1:y1 + hc, x1:x1 + wc].contiguous())
                if acc is None:
                    acc = ops._scratch((N, H, W, logits.shape[1]), logits.device, F32).zero_()
                ops.seg_window_accumulate(logits, self.out_channels, N, h, w, acc, y1, x1, hc, wc)
        return acc, cy.to(acc.device), cx.to(acc.device)

    def inference(self, inputs):
        if _cfg(self.test_cfg, "mode", "whole") == "slide":
            return self.slide_inference(inputs)
        return self.whole_inference(inputs)

    @torch.no_grad()
    def predict(self, inputs, ori_shape=None, padding=None, return_logits=False, metric=None, labels=None):
        """-> pred (N, H, W) uint8 (, seg_logits (N, K, H, W) f32 with return_logits).  padding = (left, right, top, bottom) is cut off, then the logits
        are resized to ori_shape when that differs, then the arg-max (mmseg's postprocess_result order).  With `metric` (an IoUMetric) and `labels`
        (N, H, W) the areas are counted in the arg-max launch."""
        if (metric is None) != (labels is None):
            raise ValueError("predict: metric and labels go together")
        was_training = self.training
        self.eval()
        try:
            acc, cy, cx = self.inference(inputs)
        finally:
            self.train(was_training)
        K = self.out_channels
        N, H, W, Kp = acc.shape
        pl, pr, pt, pb = (int(v) for v in (padding if padding is not None else (0, 0, 0, 0)))
        Hc, Wc = H - pt - pb, W - pl - pr
        if min(pl, pr, pt, pb) < 0 or Hc <= 0 or Wc <= 0:
            raise ValueError("predict: padding %s does not fit the %d x %d image" % ((pl, pr, pt, pb), H, W))
        Ho, Wo = (Hc, Wc) if ori_shape is None else (int(ori_shape[0]), int(ori_shape[1]))
        if (Hc, Wc) != (H, W) or (Ho, Wo) != (Hc, Wc):
            if cy is not None:      # the resize needs the averaged logits: divide in place
                ops.seg_argmax_areas(acc, K, cy, cx, write_back=True)
                cy = cx = None
            if (Hc, Wc) != (H, W):
                acc = acc[:, pt:H - pb, pl:W - pr, :].contiguous()
            if (Ho, Wo) != (Hc, Wc):
                out = ops._scratch((N, Ho, Wo, Kp), acc.device, F32)
                ops.resize_bilinear_fwd(acc.view(N * Hc * Wc, Kp), out.view(N * Ho * Wo, Kp), N, Hc, Wc, Ho, Wo)
                acc = out
        pred = ops._scratch((N, Ho, Wo), acc.device, torch.uint8)
        seg = ops._scratch((N, K, Ho, Wo), acc.device, F32) if return_logits else None
        if metric is not None:
            metric.process_logits(acc, labels, cy, cx, pred, seg)
        else:
            ops.seg_argmax_areas(acc, K, cy, cx, pred, seg)
        return (pred, seg) if return_logits else pred

    def loss(self, inputs, labels):
        return self.decode_head.loss(self.extract_feat(inputs), labels)
