"""Torch restatement of the reference's sliding-window inference and IoU metric (Multi-Task_Pretrain/semantic_segmentation/encoder_decoder.py:253-310,
metric.py:164-286), for the tests of mtp_amd.segmentors / mtp_amd.evaluation.  Plain helper module (no tests, no fixtures); pinned against the
reference's own output by fixture f18 (tests/test_seg_eval_host.py).
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F


def slide_windows(h_img, w_img, crop, stride):
    """the reference's double loop -> [(y1, x1)] in launch order and count_mat (h_img, w_img) int64"""
    (h_crop, w_crop), (h_stride, w_stride) = crop, stride
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    wins, count = [], torch.zeros(h_img, w_img, dtype=torch.int64)
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1, x1 = h_idx * h_stride, w_idx * w_stride
            y2, x2 = min(y1 + h_crop, h_img), min(x1 + w_crop, w_img)
            y1, x1 = max(y2 - h_crop, 0), max(x2 - w_crop, 0)
            wins.append((y1, x1))
            count[y1:y2, x1:x2] += 1
    return wins, count


def torch_slide_inference(inputs, encode_decode, crop, stride, K):
    """inputs (N, C, H, W); encode_decode(crop image) -> (N, K, h_crop, w_crop).  -> (seg_logits = preds / count_mat, preds, count_mat)"""
    N, _, H, W = inputs.shape
    wins, count = slide_windows(H, W, crop, stride)
    preds = inputs.new_zeros((N, K, H, W))
    for y1, x1 in wins:
        y2, x2 = y1 + crop[0], x1 + crop[1]
        preds += F.pad(encode_decode(inputs[:, :, y1:y2, x1:x2]), (x1, W - x2, y1, H - y2))
    count = count.to(inputs.dtype)[None, None]
    assert (count == 0).sum() == 0
    return preds / count, preds, count


def torch_slide_from_lowres(lowres, crop, stride, H, W):
    """the same loop on recorded per-window low-resolution logits [(N, K, h, w)] (launch order), each resized to the crop as decode_head.predict does"""
    wins, count = slide_windows(H, W, crop, stride)
    assert len(wins) == len(lowres)
    preds = lowres[0].new_zeros((lowres[0].shape[0], lowres[0].shape[1], H, W))
    for (y1, x1), lr in zip(wins, lowres):
        y2, x2 = y1 + crop[0], x1 + crop[1]
        preds += F.pad(F.interpolate(lr, size=crop, mode="bilinear", align_corners=False), (x1, W - x2, y1, H - y2))
    count = count.to(preds.dtype)[None, None]
    return preds / count, preds, count


def standin_encode_decode(weight, crop):
    """the fixture's stand-in for backbone + head, a pure function of the crop: a stride-4 conv to K channels resized to the crop.  With integer
    images and weights every value is a multiple of 1 / 64 -- exact in float64 whatever the summation order"""
    def fn(img, *_):
        return F.interpolate(F.conv2d(img, weight, stride=4), size=crop, mode="bilinear", align_corners=False)
    return fn


def torch_areas(pred, label, K, ignore_index=255):
    """metric.py:185-199 -> (3, K) int64 (intersect, pred, label)"""
    mask = label != ignore_index
    p, l = pred[mask], label[mask]
    h = [torch.histc(t.float(), bins=K, min=0, max=K - 1) for t in (p[p == l], p, l)]
    return torch.stack(h).long()


def torch_metrics(intersect, union, pred, label, metrics=("mIoU",), nan_to_num=None, beta=1):
    """metric.py:203-286 on float64 tensors -> OrderedDict of float64 tensors"""
    I, U, P, L = (torch.as_tensor(t).double() for t in (intersect, union, pred, label))
    ret = OrderedDict(aAcc=I.sum() / L.sum())
    for m in metrics:
        if m == "mIoU":
            ret["IoU"], ret["Acc"] = I / U, I / L
        elif m == "mDice":
            ret["Dice"], ret["Acc"] = 2 * I / (P + L), I / L
        elif m == "mFscore":
            pr, rc = I / P, I / L
            ret["Fscore"] = (1 + beta ** 2) * (pr * rc) / ((beta ** 2 * pr) + rc)
            ret["Precision"], ret["Recall"] = pr, rc
    if nan_to_num is not None:
        ret = OrderedDict((k, torch.nan_to_num(v, nan=float(nan_to_num), posinf=None, neginf=None)) for k, v in ret.items())
    return ret


FAMILIES = (("mIoU",), ("mDice",), ("mFscore",), ("mIoU", "mDice", "mFscore"))
# fixture f18's sliding-window geometries: (image, crop, stride).  'a': a clamped last column window (origins 0, 32, 40: counts {1, 2, 3, 4, 6}); 'b': stride < crop / 2, counts up to 9
F18_GEOMS = {"a": ((56, 88), (32, 48), (24, 32)), "b": ((50, 60), (32, 32), (12, 14))}
