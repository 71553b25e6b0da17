"""GPU: the box half of Mask R-CNN (csrc/hbox_head.hip, mtp_amd.ops.hbox_* / hrpn_* / hroi_*, DeltaXYWHBBoxCoder, MTP_IS_RPNHead,
MTP_IS_Shared2FCBBoxHead, MTP_IS_BBoxRoIHead), every op buffer out of a guard.Arena (poisoned outputs, guards on both sides, frozen inputs, the
wrappers' own workspaces included).  The references are tests/hbox_ref.py in float64 on the inputs of tests/hbox_cases.py, whose conditions
tests/test_hbox_host.py asserts, and fixture f26 (the reference's own heads, tests/golden/make_hbox_half.py) where it records the step.
  1. the coder: encode, decode with both clamps, one max_shape and a per-row table;
  2. mtp_hrpn_loss: losses per level, gradients zero off the sampled anchors, L1 sign, two calls bit-identical, counts changed on the device;
  3. mtp_hrpn_proposals: scores, clipped boxes, level ids and the size flag, a box clipped to zero width dropped at min_bbox_size 0;
  4. mtp_hroi_loss: both regression targets, the dense gradient out of a poisoned buffer, wide rows, K on either side of the wave width, a single
     row, R_total = 0, L1 at exact equality, a positive without a class, counts changed on the device;
  5. mtp_hroi_predict: scores, K boxes per RoI clipped and rescaled, flags exact, K on either side of the wave width;
  6. the heads: losses and gradients of both under set_sync_debug_mode('error'), proposals and detections exact, both heads' layers in bf16;
  7. end to end, training and test time, into the mask branch.
Exact: labels, kept indices, valid, flags, level ids, detection labels.  Every float: 4 x the error of the float32 restatement against float64
(floor 1e-6), computed here; both numbers are recorded."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import guard
import hbox_cases as HC
import hbox_ref as R
import mask_cases as MC
import rpn_ref
from conftest import record_parity
from mtp_amd import MODELS, ops
from mtp_amd.task_modules import DeltaXYWHBBoxCoder

pytestmark = pytest.mark.gpu
ARENA = None
F64, F32 = np.float64, np.float32


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    global ARENA
    ARENA = a = guard.Arena("cuda")
    monkeypatch.setattr(ops, "_scratch", a.scratch)
    yield a
    ARENA = None
    torch.cuda.synchronize()
    try:
        a.check()
    finally:
        a.close()


def dev(a):
    """an op INPUT on the device, frozen"""
    return ARENA.frozen(ARENA.like(torch.as_tensor(np.ascontiguousarray(a))))


def err_of(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a.astype(F64) - ref).max()) if ref.size else 0.0


def held(tag, out, ref64, ref32):
    """4 x the float32 CPU error of the restatement against float64, floor 1e-6"""
    ref64 = np.asarray(ref64, F64)
    err, e32 = err_of(out, ref64), err_of(np.asarray(ref32), ref64)
    record_parity("hbox", tag, err)
    record_parity("hbox", "hbox_ref_f32_cpu_" + tag, e32)
    print("%s: err %.3e, float32 restatement %.3e" % (tag, err, e32))
    assert tuple(out.shape) == ref64.shape and err < max(4 * e32, 1e-6), (tag, err, e32)


def both(fn, *args, **kw):
    """the restatement in float64 and in float32 on the same inputs"""
    return fn(*args, dtype=F64, **kw), fn(*args, dtype=F32, **kw)


# ------------------------------------------------------------------------------------------------------------------- 1. the coder
def coder_inputs(n, seed):
    rng = np.random.default_rng(seed)
    c, wh = rng.uniform(10, 54, (n, 2)), rng.uniform(4, 40, (n, 2))
    p = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    c2, wh2 = c + rng.uniform(-5, 5, (n, 2)), wh * rng.uniform(0.6, 1.6, (n, 2))
    g = np.concatenate([c2 - wh2 / 2, c2 + wh2 / 2], 1).astype(F32)
    return p, g


@pytest.mark.parametrize("n", [1, 65, 600])
def test_coder_encode(n):
    p, g = coder_inputs(n, 10 + n)
    for tag, means, stds in (("", HC.ROI_MEANS, HC.ROI_STDS), ("means_", (0.1, -0.2, 0.3, 0.05), (0.5, 0.5, 0.25, 0.3))):
        out = ops.hbox_delta_encode(dev(p), dev(g), means, stds, out=ARENA.empty(n, 4))
        r64, r32 = both(R.encode, p, g, means, stds)
        held("encode_%s%d" % (tag, n), out, r64, r32)


@pytest.mark.parametrize("n", [1, 65, 600])
def test_coder_decode(n):
    rng = np.random.default_rng(20 + n)
    p = coder_inputs(n, 30 + n)[0]
    d = (rng.normal(0, 1.0, (n, 4)) * np.array([1.5, 1.5, 2, 2])).astype(F32)
    if n > 8:      # both clamps: sizes beyond exp(+-|log(16 / 1000)|) / std, and deltas that move the box over every border
        d[:4, 2], d[:4, 3] = [45, -45, 25, -21], [-45, 45, -25, 21]
        d[4:8, 0], d[4:8, 1] = [300, -300, 0, 0], [0, 0, 300, -300]
    r64, r32 = both(R.decode, p, d, HC.ROI_MEANS, HC.ROI_STDS)
    held("decode_%d" % n, ops.hbox_delta_decode(dev(p), dev(d), HC.ROI_MEANS, HC.ROI_STDS, out=ARENA.empty(n, 4)), r64, r32)
    shapes = np.array([[64, 64], [40, 56], [48, 32]], F32)
    ids = rng.integers(0, 3, n).astype(np.int64)
    r64, r32 = both(R.decode, p, d, HC.ROI_MEANS, HC.ROI_STDS, max_shape=shapes[ids])
    out = ops.hbox_delta_decode(dev(p), dev(d), HC.ROI_MEANS, HC.ROI_STDS, max_shapes=dev(shapes), image_ids=dev(ids), out=ARENA.empty(n, 4))
    held("decode_clip_%d" % n, out, r64, r32)
    o = out.cpu().numpy()
    assert (o >= 0).all() and (o[:, 0::2] <= shapes[ids][:, 1:2]).all() and (o[:, 1::2] <= shapes[ids][:, 0:1]).all()
    assert n < 9 or ((o[:, 2] == shapes[ids][:, 1]).any() and (o[:, 0] == 0).any() and (o[:, 3] == shapes[ids][:, 0]).any() and (o[:, 1] == 0).any())
    r64, r32 = both(R.decode, p, d, HC.ROI_MEANS, HC.ROI_STDS, max_shape=(40, 56), wh_ratio_clip=0.1)      # one shape for all rows, another clip
    out = ops.hbox_delta_decode(dev(p), dev(d), HC.ROI_MEANS, HC.ROI_STDS, max_shapes=dev(shapes[1:2]), wh_ratio_clip=0.1, out=ARENA.empty(n, 4))
    held("decode_one_shape_%d" % n, out, r64, r32)


# ------------------------------------------------------------------------------------------------------------------- 2. the RPN loss
def rpn_inputs(name):
    """the float32 maps of the case's reference run and its float64 sample lists, as the kernel takes them"""
    ref = HC.reference(name)["rpn"]
    cls, reg = [m.astype(F32) for m in ref["cls"]], [m.astype(F32) for m in ref["reg"]]
    S = HC.RPN_NUM
    samples, sgt = np.zeros((HC.BATCH, S), np.int64), -np.ones((HC.BATCH, S), np.int64)
    n_pos, n_neg, off = [], [], 0
    for b, s in enumerate(ref["samples"]):
        idx = np.concatenate([s["pos"], s["neg"]])
        samples[b, :len(idx)] = idx
        sgt[b, :len(s["pos"])] = s["pos_gt"] + off
        n_pos.append(len(s["pos"]))
        n_neg.append(len(s["neg"]))
        off += len(HC.case(name)["gts"][b])
    return cls, reg, samples, sgt, np.asarray(n_pos, np.int64), np.asarray(n_neg, np.int64), ref["samples"]


def rpn_restated(name, cls, reg, sm, dtype, avg_factor=None):
    gts = HC.case(name)["gts"]
    return R.rpn_loss(cls, reg, HC.SIZES, HC.A, HC.priors(F32), gts, [s["pos"] for s in sm], [s["pos_gt"] for s in sm], [s["neg"] for s in sm],
                      HC.RPN_MEANS, HC.RPN_STDS, dtype=dtype, avg_factor=avg_factor)


@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_rpn_loss(name):
    cls, reg, samples, sgt, n_pos, n_neg, sm = rpn_inputs(name)
    gts = np.concatenate(HC.case(name)["gts"]).reshape(-1, 4)
    t_cls, t_reg = [ops.rpn_map_nchw(dev(m)) for m in cls], [ops.rpn_map_nchw(dev(m)) for m in reg]
    t_pr, t_gts = dev(HC.priors(F32)), dev(gts) if len(gts) else torch.zeros(0, 4, device="cuda")
    t_s, t_g, t_np, t_nn = dev(samples), dev(sgt), ARENA.like(torch.as_tensor(n_pos)), ARENA.like(torch.as_tensor(n_neg))

    def run():
        dcls, dreg = [ARENA.zeros(*m.shape) for m in cls], [ARENA.zeros(*m.shape) for m in reg]
        lc, lb = ops.hrpn_loss(t_cls, t_reg, HC.SIZES, HC.A, t_pr, t_gts, t_s, t_g, t_np, t_nn, HC.RPN_MEANS, HC.RPN_STDS,
                               dcls=[ops.rpn_map_nchw(d) for d in dcls], dreg=[ops.rpn_map_nchw(d) for d in dreg], loss_cls=ARENA.empty(len(cls)),
                               loss_bbox=ARENA.empty(len(cls)))
        return lc, lb, dcls, dreg
    lc, lb, dcls, dreg = run()
    r64, r32 = rpn_restated(name, cls, reg, sm, F64), rpn_restated(name, cls, reg, sm, F32)
    held(name + "_loss_rpn_cls", lc, r64[0], r32[0])
    held(name + "_loss_rpn_bbox", lb, r64[1], r32[1])
    for l in range(len(cls)):
        held("%s_rpn_dcls_%d" % (name, l), dcls[l], r64[2][l], r32[2][l])
        held("%s_rpn_dreg_%d" % (name, l), dreg[l], r64[3][l], r32[3][l])
        assert not dcls[l].cpu().numpy()[r64[2][l] == 0].any() and not dreg[l].cpu().numpy()[r64[3][l] == 0].any()
        assert np.array_equal(np.sign(dreg[l].cpu().numpy()), np.sign(r64[3][l]))      # L1: the sign is the gradient
    if name == "nopos":
        assert not float(lb.sum()) and float(lc.sum()) > 0 and not any(d.any() for d in dreg)
    again = run()
    assert torch.equal(again[0], lc) and torch.equal(again[1], lb) and all(torch.equal(a, b) for a, b in zip(again[2] + again[3], dcls + dreg))
    # the counts are read on the device: one positive and one negative fewer per image, nothing reallocated
    t_np.copy_(torch.clamp(t_np - 1, min=0))
    t_nn.copy_(torch.clamp(t_nn - 1, min=0))
    if name == "full":
        # the slots are positional: with n_pos - 1 the last positive's slot is read as the first negative
        cut = [dict(pos=s["pos"][:-1], pos_gt=s["pos_gt"][:-1], neg=np.concatenate([s["pos"][-1:], s["neg"][:-2]])) for s in sm]
        lc2, lb2, dcls2, dreg2 = run()
        q64, q32 = rpn_restated(name, cls, reg, cut, F64), rpn_restated(name, cls, reg, cut, F32)
        held(name + "_loss_rpn_cls_fewer", lc2, q64[0], q32[0])
        held(name + "_loss_rpn_bbox_fewer", lb2, q64[1], q32[1])
        assert not torch.equal(lc2, lc)


# ------------------------------------------------------------------------------------------------------------------- 3. the proposals
def proposal_run(cls, reg, min_size):
    """the kernel on maps (B, ., H, W) float32 -> its outputs and, per image, the restated lists in both precisions"""
    B = cls[0].shape[0]
    keep = [rpn_ref.topk_per_level([m[b] for m in cls], HC.PROPOSAL["nms_pre"]) for b in range(B)]
    counts = [len(k) for k in keep[0]]
    T = sum(counts)
    t_keep = dev(np.stack([np.concatenate(k) for k in keep]).astype(np.int64))
    out = (ARENA.empty(B, T), ARENA.empty(B, T, 4), ARENA.empty(B, T, dtype=torch.int64), ARENA.empty(B, T, dtype=torch.uint8))
    shapes = dev(np.array([HC.IMG] * B, F32))
    scores, boxes, ids, valid = ops.hrpn_proposals([ops.rpn_map_nchw(dev(m)) for m in cls], [ops.rpn_map_nchw(dev(m)) for m in reg], HC.SIZES, HC.A,
                                                   dev(HC.priors(F32)), t_keep, counts, HC.RPN_MEANS, HC.RPN_STDS, shapes, min_size, out=out)
    lists = []
    for b in range(B):
        args = ([m[b] for m in cls], [m[b] for m in reg], HC.priors(F32), HC.SIZES, HC.A, keep[b], HC.RPN_MEANS, HC.RPN_STDS, HC.IMG)
        lists.append((R.rpn_decode_kept(*args, dtype=F64), R.rpn_decode_kept(*args, dtype=F32)))
    return scores, boxes, ids, valid, lists


@pytest.mark.parametrize("name", ["full", "planted"])
def test_rpn_proposals(name):
    if name == "planted":
        cls, reg, (pb, pl, pidx) = HC.planted()
    else:
        cls, reg = rpn_inputs(name)[:2]
    for min_size in (0.0, -1.0, 6.0):
        scores, boxes, ids, valid, lists = proposal_run(cls, reg, min_size)
        for b, ((s64, b64, i64), (s32, b32, _)) in enumerate(lists):
            held("%s_prop_scores_%d" % (name, b), scores[b], s64, s32)
            held("%s_prop_boxes_%d" % (name, b), boxes[b], b64, b32)
            assert ids[b].tolist() == i64.tolist()
            want = ((b64[:, 2] - b64[:, 0]) > min_size) & ((b64[:, 3] - b64[:, 1]) > min_size)
            assert valid[b].bool().tolist() == want.tolist()
            assert min_size >= 0 or want.all()
            o = boxes[b].cpu().numpy()
            assert (o >= 0).all() and (o[:, 0::2] <= HC.IMG[1]).all() and (o[:, 1::2] <= HC.IMG[0]).all()
        if name == "planted" and min_size == 0.0:      # the planted anchor: clipped to zero width, dropped
            at = int(np.nonzero(rpn_ref.topk_per_level([m[pb] for m in cls], HC.PROPOSAL["nms_pre"])[pl] == pidx)[0][0])
            assert boxes[pb, at, 0] == HC.IMG[1] and boxes[pb, at, 2] == HC.IMG[1] and not valid[pb, at]


# ------------------------------------------------------------------------------------------------------------------- 4. the RoI loss
def roi_inputs(name):
    ref = HC.reference(name)["roi"]
    s = ref["lists"]
    return ref["cls"].astype(F32), ref["reg"].astype(F32), s


def roi_loss_run(cls, reg, K, s, reg_target, ld_extra=0, means=HC.ROI_MEANS, stds=HC.ROI_STDS, counts=None):
    """-> losses (3), dcls (R, K + 1), dreg (R, 4 K) out of poisoned buffers; ld_extra: the rows are column slices of wider buffers"""
    Rn = len(cls)
    c0 = -(-(K + 1) // 4) * 4      # the deltas start on a 16-byte boundary
    wide = c0 + 4 * K + ld_extra
    buf, dbuf = ARENA.wide(Rn, wide), ARENA.wide(Rn, wide)
    t_cls, t_reg = ARENA.cols(buf, 0, K + 1), ARENA.cols(buf, c0, c0 + 4 * K)
    t_cls.copy_(torch.as_tensor(cls))
    t_reg.copy_(torch.as_tensor(reg))
    ARENA.frozen(buf)
    dcls, dreg = ARENA.cols(dbuf, 0, K + 1), ARENA.cols(dbuf, c0, c0 + 4 * K)
    gts = dev(s["gts"]) if len(s["gts"]) else torch.zeros(0, 4, device="cuda")
    labels = dev(s["gt_labels"]) if len(s["gts"]) else torch.zeros(0, dtype=torch.int64, device="cuda")
    n_pos, n_neg = counts if counts is not None else (dev(s["n_pos"]), dev(s["n_neg"]))
    losses = ops.hroi_loss(t_cls, t_reg, K, dev(np.ascontiguousarray(s["rois"][:, 1:])), gts, labels, dev(s["sample_gt"]), n_pos, n_neg, means, stds, reg_target,
                           dcls=dcls, dreg=dreg, losses=ARENA.empty(3))
    return losses, dcls, dreg


def roi_restated(cls, reg, K, s, reg_target, dtype, n_pos=None, n_neg=None):
    return R.roi_loss(cls, reg, K, s["rois"][:, 1:], s["gts"], s["gt_labels"], s["sample_gt"], s["n_pos"] if n_pos is None else n_pos,
                      s["n_neg"] if n_neg is None else n_neg, HC.ROI_MEANS, HC.ROI_STDS, reg_target, dtype=dtype)


def check_roi_loss(tag, got, r64, r32, K):
    losses, dcls, dreg = got
    for i, k in enumerate(("loss_cls", "loss_bbox", "acc")):
        held("%s_%s" % (tag, k), losses[i].reshape(1), np.asarray(r64[k]).reshape(1), np.asarray(r32[k]).reshape(1))
    held(tag + "_dcls", dcls, r64["dcls"], r32["dcls"])
    held(tag + "_dreg", dreg, r64["dreg"], r32["dreg"])
    d = dreg.cpu().numpy()
    assert not np.isnan(d).any() and not d[r64["dreg"] == 0].any()      # dense: zeros in every column that is not the label's, written
    assert np.array_equal(np.sign(d), np.sign(r64["dreg"]))
    pos = (r64["labels"] >= 0) & (r64["labels"] < K)
    assert int((d != 0).any(1).sum()) <= int(pos.sum())


@pytest.mark.parametrize("reg_target", ["reference", "encoded"])
@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_roi_loss(name, reg_target):
    cls, reg, s = roi_inputs(name)
    got = roi_loss_run(cls, reg, HC.K, s, reg_target, ld_extra=4)
    check_roi_loss("%s_%s" % (name, reg_target), got, roi_restated(cls, reg, HC.K, s, reg_target, F64), roi_restated(cls, reg, HC.K, s, reg_target, F32), HC.K)
    again = roi_loss_run(cls, reg, HC.K, s, reg_target, ld_extra=4)
    assert all(torch.equal(a, b) for a, b in zip(again, got))      # two calls: the same bits
    if name == "full":
        assert not s["valid"].all() and float(got[0][1]) > 0      # padded slots, and a box term
    if name != "full":
        assert (s["n_pos"] == 0).any()


def test_roi_loss_counts_changed_on_the_device():
    cls, reg, s = roi_inputs("full")
    n_pos, n_neg = ARENA.like(torch.as_tensor(s["n_pos"])), ARENA.like(torch.as_tensor(s["n_neg"]))
    first = roi_loss_run(cls, reg, HC.K, s, "reference", counts=(n_pos, n_neg))[0].clone()
    n_neg.copy_(torch.clamp(n_neg - 3, min=0))      # nothing reallocated: the same two tensors
    got = roi_loss_run(cls, reg, HC.K, s, "reference", counts=(n_pos, n_neg))
    fewer = np.maximum(s["n_neg"] - 3, 0)
    check_roi_loss("fewer", got, roi_restated(cls, reg, HC.K, s, "reference", F64, n_neg=fewer), roi_restated(cls, reg, HC.K, s, "reference", F32, n_neg=fewer), HC.K)
    assert not torch.equal(first, got[0])
    n_pos.zero_()
    n_neg.zero_()                                   # R_total = 0: the losses and every gradient are 0
    losses, dcls, dreg = roi_loss_run(cls, reg, HC.K, s, "encoded", counts=(n_pos, n_neg))
    assert not losses.any() and not dcls.any() and not dreg.any()


def seam_case(K, rows, seed):
    """random rows for a head of K classes: two images of `rows` slots, a third of them positive, some padding"""
    rng = np.random.default_rng(seed)
    B, S = (1, 1) if rows == 1 else (2, rows)
    n = B * S
    G = 5
    c, wh = rng.uniform(16, 48, (G, 2)), rng.uniform(10, 30, (G, 2))
    gts = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    gt_labels = rng.integers(0, K, G).astype(np.int64)
    gt_labels[0] = K - 1      # the last class: the last 16 bytes of a row of deltas
    n_pos = np.full(B, max(1, S // 3), np.int64)
    n_neg = np.asarray([S - n_pos[0]] + [max(S - n_pos[0] - 2, 0)] * (B - 1), np.int64)[:B]
    sgt = -np.ones((B, S), np.int64)
    for b in range(B):
        sgt[b, :n_pos[b]] = rng.integers(0, G, n_pos[b])
    sgt[0, 0] = 0
    rois = np.zeros((n, 5), F32)
    rois[:, 0] = np.repeat(np.arange(B), S)
    ctr, rwh = rng.uniform(16, 48, (n, 2)), rng.uniform(8, 30, (n, 2))
    rois[:, 1:] = np.concatenate([ctr - rwh / 2, ctr + rwh / 2], 1)
    for b in range(B):      # a positive's RoI lies on its gt, as the assigner sees to (IoU >= 0.5): the encoded targets are O(1), where the
        for j in range(n_pos[b]):      # absolute floor of the bound is a few ulp and not a fraction of one
            rois[b * S + j, 1:] = gts[sgt[b, j]] + rng.uniform(-1.5, 1.5, 4)
    cls = rng.normal(0, 2.0, (n, K + 1)).astype(F32)
    reg = rng.normal(0, 0.5, (n, 4 * K)).astype(F32)
    if K > 2:      # the first maximum of a row is the arg-max: an exact tie between two columns of one lane's trips and of two lanes
        cls[0, 1] = cls[0, K] = np.float32(9.0)
    s = dict(rois=rois, sample_gt=sgt, n_pos=n_pos, n_neg=n_neg, gts=gts, gt_labels=gt_labels)
    return cls, reg, s


@pytest.mark.parametrize("rows", [1, 9])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
def test_roi_loss_class_seams(K, rows):
    """K + 1 logits on either side of the wave width (64 lanes), ld_reg = 4 K, one row and more than one workgroup's four"""
    cls, reg, s = seam_case(K, rows, 100 + K)
    for t in ("reference", "encoded"):
        got = roi_loss_run(cls, reg, K, s, t)
        check_roi_loss("seam_%d_%d_%s" % (K, rows, t), got, roi_restated(cls, reg, K, s, t, F64), roi_restated(cls, reg, K, s, t, F32), K)


def test_roi_loss_l1_at_equality_and_a_positive_without_a_class():
    cls, reg, s = seam_case(3, 9, 7)
    s = dict(s, gt_labels=s["gt_labels"].copy(), sample_gt=s["sample_gt"].copy())
    lab = int(s["gt_labels"][0])
    reg[0, 4 * lab:4 * lab + 4] = [1.0, 1.0, 0.5, 1.0]      # slot 0 is a positive of gt 0: three of its four terms sit on the target 1.0
    s["gt_labels"][1] = 3                                   # a label outside [0, K): the positives of gt 1 are padding
    s["sample_gt"][0, 1], s["sample_gt"][1, 0] = 1, 17     # ... and a gt row outside [0, G)
    losses, dcls, dreg = roi_loss_run(cls, reg, 3, s, "reference")
    r64, r32 = roi_restated(cls, reg, 3, s, "reference", F64), roi_restated(cls, reg, 3, s, "reference", F32)
    check_roi_loss("equality", (losses, dcls, dreg), r64, r32, 3)
    row = dreg[0, 4 * lab:4 * lab + 4].tolist()
    assert row[0] == 0.0 and row[1] == 0.0 and row[3] == 0.0 and row[2] < 0      # sign(0) = 0, as torch has it
    assert r64["labels"][1] == -1 and r64["labels"][9] == -1 and not dcls[1].any() and not dreg[1].any() and not dcls[9].any()


# ------------------------------------------------------------------------------------------------------------------- 5. predict
def predict_run(cls, reg, K, rois, shapes, inv, thr):
    Rn = len(cls)
    c0 = -(-(K + 1) // 4) * 4
    buf = ARENA.wide(Rn, c0 + 4 * K)
    t_cls, t_reg = ARENA.cols(buf, 0, K + 1), ARENA.cols(buf, c0, c0 + 4 * K)
    t_cls.copy_(torch.as_tensor(cls))
    t_reg.copy_(torch.as_tensor(reg))
    ARENA.frozen(buf)
    out = (ARENA.empty(Rn, K), ARENA.empty(Rn, K, 4), ARENA.empty(Rn, K, dtype=torch.uint8))
    return ops.hroi_predict(t_cls, t_reg, K, dev(rois), HC.ROI_MEANS, HC.ROI_STDS, dev(shapes), None if inv is None else dev(inv), thr, out=out)


def check_predict(tag, got, cls, reg, K, rois, shapes, inv, thr):
    scores, boxes, flags = got
    b = rois[:, 0].astype(np.int64)
    args = (cls, reg, K, rois[:, 1:], HC.ROI_MEANS, HC.ROI_STDS, shapes[b], None if inv is None else inv[b])
    (s64, b64), (s32, b32) = R.roi_predict(*args, dtype=F64), R.roi_predict(*args, dtype=F32)
    held(tag + "_scores", scores, s64, s32)
    held(tag + "_boxes", boxes, b64, b32)
    assert np.abs(s64 - thr).min() > 1e-6 and flags.bool().cpu().numpy().tolist() == (s64 > thr).tolist()


@pytest.mark.parametrize("rescale", [False, True])
def test_roi_predict(rescale):
    ref = HC.reference("full")
    cls, reg, rois = ref["tcls"].astype(F32), ref["treg"].astype(F32), ref["test_rois"]
    shapes = np.array([HC.IMG] * HC.BATCH, F32)
    inv = np.array([[1.0 / HC.SCALE_FACTOR[0], 1.0 / HC.SCALE_FACTOR[1]]] * HC.BATCH, F32) if rescale else None
    got = predict_run(cls, reg, HC.K, rois, shapes, inv, HC.RCNN["score_thr"])
    check_predict("predict_%d" % rescale, got, cls, reg, HC.K, rois, shapes, inv, HC.RCNN["score_thr"])
    o = got[1].cpu().numpy().reshape(-1, 4)
    fx, fy = (inv[0] if rescale else (1.0, 1.0))
    assert (o[:, 0] == 0).any() and (o[:, 1] == 0).any() and (o[:, 2] == np.float32(HC.IMG[1]) * np.float32(fx)).any() and (o[:, 3] == np.float32(HC.IMG[0]) * np.float32(fy)).any()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
def test_roi_predict_class_seams(K):
    cls, reg, s = seam_case(K, 9, 200 + K)
    rois = s["rois"].copy()
    rois[3, 1:] = [-9.0, 20.0, 30.0, 70.0]      # sticking out on the left and below
    shapes = np.array([[64, 64], [48, 56]], F32)
    inv = np.array([[0.8, 1.25], [0.5, 2.0]], F32)
    v = np.sort(R.roi_predict(cls, reg, K, rois[:, 1:], HC.ROI_MEANS, HC.ROI_STDS, shapes[rois[:, 0].astype(int)])[0].reshape(-1))
    wide = np.nonzero(np.diff(v) > 2e-5)[0]      # the threshold: the middle of a gap of the float64 scores, the one nearest their median
    i = wide[np.argmin(np.abs(wide - len(v) // 2))]
    thr = float((v[i] + v[i + 1]) / 2)
    got = predict_run(cls, reg, K, rois, shapes, inv, thr)
    check_predict("predict_seam_%d" % K, got, cls, reg, K, rois, shapes, inv, thr)


# ------------------------------------------------------------------------------------------------------------------- 6. the heads
def make_rpn(c, precision="fp32", in_channels=HC.C, feat_channels=HC.FEAT):
    head = MODELS.build(dict(
        type="MTP_IS_RPNHead", in_channels=in_channels, feat_channels=feat_channels,
        anchor_generator=dict(type="AnchorGenerator", scales=list(HC.SCALES), ratios=list(HC.RATIOS), strides=list(HC.STRIDES)),
        bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=list(HC.RPN_MEANS), target_stds=list(HC.RPN_STDS)),
        loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_bbox=dict(type="L1Loss", loss_weight=1.0),
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", **HC.RPN_ASSIGNER),
                       sampler=dict(type="RandomSampler", num=HC.RPN_NUM, pos_fraction=HC.RPN_POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=False),
                       allowed_border=-1, pos_weight=-1, debug=False),
        test_cfg=dict(HC.PROPOSAL), precision=precision)).cuda()
    head.load_state_dict({k: torch.as_tensor(v) for k, v in c["rpn"].items()})
    return head


def make_roi(c, precision="fp32", num_classes=HC.K, reg_target="reference"):
    cfg = dict(
        type="MTP_IS_BBoxRoIHead",
        bbox_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=HC.P, sampling_ratio=0), out_channels=HC.C,
                                featmap_strides=list(HC.ROI_STRIDES)),
        bbox_head=dict(type="MTP_IS_Shared2FCBBoxHead", in_channels=HC.C, fc_out_channels=HC.FC_OUT, roi_feat_size=HC.P,
                       bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=list(HC.ROI_MEANS), target_stds=list(HC.ROI_STDS)),
                       reg_class_agnostic=False, loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                       loss_bbox=dict(type="L1Loss", loss_weight=1.0), reg_target=reg_target, precision=precision),
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", **HC.ROI_ASSIGNER),
                       sampler=dict(type="RandomSampler", num=HC.ROI_NUM, pos_fraction=HC.ROI_POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=True),
                       pos_weight=-1, debug=False),
        test_cfg=dict(HC.RCNN))
    if num_classes is not None:
        cfg["bbox_head"]["num_classes"] = num_classes
    head = MODELS.build(cfg).cuda()
    head.load_state_dict({"bbox_head." + k: torch.as_tensor(v) for k, v in c["roi"].items() if num_classes is not None or k.startswith("shared_fcs.")})
    return head


def make_mask(c):
    head = MODELS.build(dict(
        type="MTP_IS_StandardRoIHead",
        mask_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=MC.OUT, sampling_ratio=0), out_channels=HC.C,
                                featmap_strides=list(MC.STRIDES), finest_scale=MC.FINEST),
        mask_head=dict(type="MTP_IS_FCNMaskHead", num_convs=MC.NUM_CONVS, in_channels=HC.C, conv_out_channels=MC.CONV,
                       loss_mask=dict(type="CrossEntropyLoss", use_mask=True, loss_weight=MC.LOSS_WEIGHT)),
        train_cfg=dict(mask_size=MC.M, sampler=dict(type="RandomSampler", num=HC.ROI_NUM, pos_fraction=HC.ROI_POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=True),
                       pos_weight=-1, debug=False),
        test_cfg=dict(mask_thr_binary=MC.THR))).cuda()
    head.load_state_dict({"mask_head." + k: torch.as_tensor(v) for k, v in c["mask"].items()})
    conv_logits = torch.nn.Conv2d(MC.CONV, HC.K, 1).cuda()
    with torch.no_grad():
        conv_logits.weight.copy_(torch.as_tensor(c["conv_logits"]["weight"]))
        conv_logits.bias.copy_(torch.as_tensor(c["conv_logits"]["bias"]))
    return head, conv_logits


def inputs(name):
    c = HC.case(name)
    feats = [dev(f) for f in c["feats"]]
    gts = [NS(bboxes=dev(g) if len(g) else torch.zeros(0, 4, device="cuda"), labels=dev(l) if len(l) else torch.zeros(0, dtype=torch.int64, device="cuda"))
           for g, l in zip(c["gts"], c["labels"])]
    return c, feats, gts


def picks(samples):
    return [(s["pos"], s["neg"]) for s in samples]


def no_sync(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def check_proposals(name, got, ref, yard):
    for b, p in enumerate(got):
        keep, bx, sc, _ = ref[b]
        assert p.keep.tolist() == keep.tolist() and not p.labels.any() and p.labels.dtype == torch.int64      # exact, in output order
        held("%s_proposals_%d" % (name, b), p.bboxes, bx, yard[b][1])
        held("%s_proposal_scores_%d" % (name, b), p.scores, sc, yard[b][2])


@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_rpn_head(name):
    c, feats, gts = inputs(name)
    ref, y32 = HC.reference(name)["rpn"], HC.yardstick(name)["rpn"]
    head = make_rpn(c)
    cls, reg = head(feats)
    for l in range(len(feats)):
        held("%s_rpn_cls_%d" % (name, l), cls[l], ref["cls"][l], y32["cls"][l])
        held("%s_rpn_reg_%d" % (name, l), reg[l], ref["reg"][l], y32["reg"][l])
    losses, G, dfeats = head.loss_and_grads(feats, gts, HC.METAS, sample_inds=picks(ref["samples"]))
    held(name + "_head_loss_rpn_cls", torch.stack(losses["loss_rpn_cls"]), ref["loss_cls"], y32["loss_cls"])
    held(name + "_head_loss_rpn_bbox", torch.stack(losses["loss_rpn_bbox"]), ref["loss_bbox"], y32["loss_bbox"])
    assert sorted(G) == sorted(ref["G"])
    for k in G:
        held("%s_rpn_d_%s" % (name, k), G[k], ref["G"][k], y32["G"][k])
    for l in range(len(feats)):
        held("%s_rpn_dfeat_%d" % (name, l), dfeats[l], ref["dfeats"][l], y32["dfeats"][l])
    out = no_sync(lambda: head.loss_and_grads(feats, gts, HC.METAS, generator=torch.Generator(device="cuda").manual_seed(1)))      # the slot form: no host sync
    assert all(torch.isfinite(t).all() for t in out[0]["loss_rpn_cls"] + out[0]["loss_rpn_bbox"])
    by_feat, dcls, dreg = head.loss_by_feat(cls, reg, gts, HC.METAS, sample_inds=picks(ref["samples"]), return_grads=True)
    assert torch.equal(torch.stack(by_feat["loss_rpn_cls"]), torch.stack(losses["loss_rpn_cls"]))
    for l in range(len(feats)):
        held("%s_by_feat_dreg_%d" % (name, l), dreg[l], ref["dreg"][l], y32["dreg"][l])
    check_proposals(name, head.predict(feats, HC.METAS), ref["props"], y32["props"])
    l2, props = head.loss_and_predict(feats, gts, HC.METAS, sample_inds=picks(ref["samples"]))
    assert torch.equal(torch.stack(l2["loss_rpn_bbox"]), torch.stack(losses["loss_rpn_bbox"]))
    check_proposals(name + "_lp", props, ref["props"], y32["props"])
    check_proposals(name + "_by_feat", head.predict_by_feat(cls, reg, HC.METAS), ref["props"], y32["props"])


def test_rpn_head_planted_zero_width():
    """predict_by_feat on the planted maps: the anchor whose clipped box has width exactly 0 is dropped by min_bbox_size = 0 and kept by -1"""
    cls, reg, (pb, pl, pidx) = HC.planted()
    head = make_rpn(HC.case("full"))
    t_cls, t_reg = [dev(m) for m in cls], [dev(m) for m in reg]
    at = int(np.nonzero(rpn_ref.topk_per_level([m[pb] for m in cls], HC.PROPOSAL["nms_pre"])[pl] == pidx)[0][0])
    for min_size, inside in ((0, False), (-1, True)):
        cfg = dict(HC.PROPOSAL, min_bbox_size=min_size, max_per_img=1000)
        got = head.predict_by_feat(t_cls, t_reg, HC.METAS, cfg=cfg)
        for b in range(HC.BATCH):
            want = R.rpn_proposals([m[b] for m in cls], [m[b] for m in reg], HC.priors(F32), HC.SIZES, HC.A, HC.RPN_MEANS, HC.RPN_STDS, HC.IMG, cfg["nms_pre"],
                                   cfg["max_per_img"], cfg["nms"]["iou_threshold"], min_size)
            assert got[b].keep.tolist() == want[0].tolist()
        assert (at in got[pb].keep.tolist()) == inside


BF16_IMG, BF16_CIN, BF16_FEAT, BF16_SEED, BF16_GAP = (64, 64), 8, 8, 139, 2e-6


def bf16_boundary_margin(c):
    """float64: the smallest relative distance of an output of the 3x3 convolution (bf16-rounded operands) from a bf16 rounding boundary.  The engine
    rounds that output to bf16; an element nearer to a boundary than the float32 summation error can round the other way on the device, and is then
    a whole bf16 step off: a threshold that decides bits, so the seed is chosen clear of it, like the thresholds of hbox_cases"""
    import torch.nn.functional as F

    def bf16(t):
        return t.to(torch.bfloat16).to(t.dtype)
    w, b = torch.from_numpy(c["rpn"]["rpn_conv.weight"]).double(), torch.from_numpy(c["rpn"]["rpn_conv.bias"]).double()
    m = np.inf
    for f in c["feats"]:
        z = F.conv2d(bf16(torch.from_numpy(f).double()), bf16(w), b, padding=1)
        near = bf16(z.float()).double()
        step = 2.0 ** (torch.floor(torch.log2(near.abs().clamp_min(1e-30))) - 7)
        m = min(m, float(((step / 2 - (z - near).abs()).abs() / z.abs().clamp_min(1e-30)).min()))
    return m


def bf16_rpn_case(seed=BF16_SEED):
    """inputs of the bf16 run of the RPN head at the cases' sizes.  The loss kernel takes any lists: 8 random positives with random gts and 8 random
    negatives per image.  The seed is the first whose bf16_boundary_margin exceeds BF16_GAP and whose L1 margin exceeds 1e-2 (asserted in the test)."""
    rng = np.random.default_rng(2800 + seed)
    sizes = [(-(-BF16_IMG[0] // s), -(-BF16_IMG[1] // s)) for s in HC.STRIDES]
    priors = np.concatenate([rpn_ref.grid_priors(rpn_ref.base_anchors(s, HC.SCALES, HC.RATIOS), H, W, (s, s), F64) for (H, W), s in zip(sizes, HC.STRIDES)])
    feats = [rng.normal(0, 1, (HC.BATCH, BF16_CIN, H, W)).astype(F32) for H, W in sizes]
    W_ = {"rpn_conv.weight": rng.normal(0, 0.08, (BF16_FEAT, BF16_CIN, 3, 3)), "rpn_conv.bias": rng.normal(0, 0.2, BF16_FEAT),
          "rpn_cls.weight": rng.normal(0, 0.08, (HC.A, BF16_FEAT, 1, 1)), "rpn_cls.bias": rng.normal(0, 0.2, HC.A),
          "rpn_reg.weight": rng.normal(0, 0.08, (4 * HC.A, BF16_FEAT, 1, 1)), "rpn_reg.bias": rng.normal(0, 0.2, 4 * HC.A)}
    gts, samples = [], []
    for b in range(HC.BATCH):
        ctr, wh = rng.uniform(16, 48, (3, 2)), rng.uniform(10, 30, (3, 2))
        gts.append(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F32))
        idx = rng.permutation(len(priors))[:16]
        samples.append(dict(pos=np.sort(idx[:8]), neg=np.sort(idx[8:]), pos_gt=rng.integers(0, 3, 8)))
    return dict(feats=feats, rpn={k: v.astype(F32) for k, v in W_.items()}, gts=gts, samples=samples, sizes=sizes, priors=priors)


def rpn_composition(c, rounding, tt):
    """the RPN head's convolutions, loss and backward on the CPU in tt.  rounding: the engine's 'bf16' mode (hbox_cases.rpn_maps).
    -> dict(cls, reg, loss_cls, loss_bbox, G, dfeats, margin: the smallest |pred - target| of an L1 term)"""
    def bf16(t):
        return t.to(torch.bfloat16).to(t.dtype)
    rnd = (lambda t: t + (bf16(t) - t).detach()) if rounding else None
    rgrad = (lambda t: t.register_hook(bf16) and t) if rounding else None
    dt = F64 if tt == torch.float64 else F32
    samples, sizes = c["samples"], c["sizes"]
    feats = [torch.from_numpy(f).to(tt).requires_grad_() for f in c["feats"]]
    W = {k: torch.from_numpy(v).to(tt).requires_grad_() for k, v in c["rpn"].items()}
    cls, reg = HC.rpn_maps(feats, W, rnd, rgrad)
    ncls, nreg = [m.detach().numpy() for m in cls], [m.detach().numpy() for m in reg]
    lc, lb, dcls, dreg, tgt = R.rpn_loss(ncls, nreg, sizes, HC.A, c["priors"].astype(F32), c["gts"], [s["pos"] for s in samples], [s["pos_gt"] for s in samples],
                                         [s["neg"] for s in samples], HC.RPN_MEANS, HC.RPN_STDS, dtype=dt)
    grads = torch.autograd.grad(cls + reg, list(W.values()) + feats, [torch.from_numpy(d) for d in dcls + dreg])
    margin = np.inf
    for b, s in enumerate(samples):
        lvl, y, x, a = rpn_ref.level_of(s["pos"], sizes, HC.A)
        for j in range(len(s["pos"])):
            margin = min(margin, R.l1_margin(nreg[lvl[j]][b, a[j] * 4:a[j] * 4 + 4, y[j], x[j]], tgt[b][j]))
    return dict(cls=ncls, reg=nreg, loss_cls=lc, loss_bbox=lb, G={k: g.numpy() for k, g in zip(W, grads[:len(W)])}, dfeats=[g.numpy() for g in grads[len(W):]],
                margin=margin)


def test_rpn_head_bf16_vs_cpu():
    """MTP_IS_RPNHead in 'bf16' (its two 1x1 convolutions are one GEMM of (1 + 4) A = 15 columns padded to 16) against a CPU run whose operands are
    rounded where the engine keeps bf16: maps, losses, parameter and map gradients"""
    c = bf16_rpn_case()
    truth, yard = rpn_composition(c, True, torch.float64), rpn_composition(c, True, torch.float32)
    assert truth["margin"] > 1e-2      # L1: no term of the rounded run so near its target that the kernel's sign could differ
    assert bf16_boundary_margin(c) > BF16_GAP
    head = make_rpn(c, "bf16", BF16_CIN, BF16_FEAT)
    feats = [dev(f) for f in c["feats"]]
    gts = [NS(bboxes=dev(g), labels=torch.zeros(len(g), dtype=torch.int64, device="cuda")) for g in c["gts"]]
    metas = [dict(img_shape=BF16_IMG, pad_shape=BF16_IMG)] * HC.BATCH
    cls, reg = head(feats)
    # the lists go in as they are: the gt of every positive is given, not assigned
    S = 16
    samples = dev(np.stack([np.concatenate([s["pos"], s["neg"]]) for s in c["samples"]]).astype(np.int64))
    sgt = -np.ones((HC.BATCH, S), np.int64)
    for b, s in enumerate(c["samples"]):
        sgt[b, :8] = s["pos_gt"] + 3 * b
    eng, out, ctx, mcls, mreg, sizes = head._maps(feats)
    dout = torch.zeros_like(out)
    lc, lb = ops.hrpn_loss(mcls, mreg, sizes, HC.A, dev(c["priors"].astype(F32)), dev(np.concatenate(c["gts"])), samples, dev(sgt),
                           dev(np.full(HC.BATCH, 8, np.int64)), dev(np.full(HC.BATCH, 8, np.int64)), HC.RPN_MEANS, HC.RPN_STDS,
                           dcls=[(dout,) + m[1:] for m in mcls], dreg=[(dout,) + m[1:] for m in mreg])
    G = {n: torch.zeros_like(p) for n, p in head.named_parameters()}
    dfeats = [type(eng).to_nchw(d, *g) for d, g in zip(eng.backward_maps(dout, ctx, G), ctx["geoms"])]
    assert sizes == c["sizes"] and gts and metas
    held("rpn_bf16_loss_cls", lc, truth["loss_cls"], yard["loss_cls"])
    held("rpn_bf16_loss_bbox", lb, truth["loss_bbox"], yard["loss_bbox"])
    for l in range(len(feats)):
        held("rpn_bf16_cls_%d" % l, cls[l], truth["cls"][l], yard["cls"][l])
        held("rpn_bf16_reg_%d" % l, reg[l], truth["reg"][l], yard["reg"][l])
        held("rpn_bf16_dfeat_%d" % l, dfeats[l], truth["dfeats"][l], yard["dfeats"][l])
    for k in G:
        held("rpn_bf16_d_" + k, G[k], truth["G"][k], yard["G"][k])


def roi_setup(name):
    c, feats, gts = inputs(name)
    ref, y32 = HC.reference(name), HC.yardstick(name)
    props = [NS(bboxes=dev(p[1].astype(F32))) for p in ref["rpn"]["props"]]
    return c, feats, gts, props, ref, y32


@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_roi_head_loss_and_grads(name):
    c, feats, gts, props, ref, y32 = roi_setup(name)
    r, y = ref["roi"], y32["roi"]
    head = make_roi(c)
    pick = picks(r["samples"])
    s = head.gen_sampling_results(props, gts, sample_inds=pick)
    lists = r["lists"]
    assert s["n_pos"].tolist() == lists["n_pos"].tolist() and s["n_neg"].tolist() == lists["n_neg"].tolist()
    v = torch.as_tensor(lists["valid"]).cuda()
    assert torch.equal(s["rois"][v], torch.as_tensor(lists["rois"][lists["valid"]]).cuda()) and s["sample_gt"].tolist() == lists["sample_gt"].tolist()
    want_labels = r["loss"]["reference"]["labels"]
    pos = (want_labels >= 0) & (want_labels < HC.K)
    assert s["pos"]["labels"].cpu().numpy()[pos].tolist() == want_labels[pos].tolist() and torch.equal(s["pos"]["n_pos"], s["n_pos"])      # exact
    bf, _ = head.train_bbox_forward(feats, s)
    held(name + "_bbox_feats", bf, r["x"], y["x"])
    losses, G, dfeats = head.loss_and_grads(feats, props, gts, sample_inds=pick)
    for k in ("loss_cls", "loss_bbox", "acc"):
        held("%s_head_%s" % (name, k), losses[k].reshape(1), np.asarray(r["loss"]["reference"][k]).reshape(1), np.asarray(y["loss"]["reference"][k]).reshape(1))
    assert sorted(G) == sorted("bbox_head." + k for k in r["G"]) and all(p.grad is None for p in head.parameters())
    for k in r["G"]:
        held("%s_roi_d_%s" % (name, k), G["bbox_head." + k], r["G"][k], y["G"][k])
    for l in range(len(HC.ROI_STRIDES)):
        held("%s_roi_dfeat_%d" % (name, l), dfeats[l], r["dfeats"][l], y["dfeats"][l])
    out = no_sync(lambda: head.loss_and_grads(feats, props, gts, generator=torch.Generator(device="cuda").manual_seed(1)))      # the slot form: no host sync
    assert all(torch.isfinite(t).all() for t in out[0].values())
    again = head.loss_and_grads(feats, props, gts, sample_inds=pick)
    assert all(torch.equal(again[0][k], losses[k]) for k in losses) and all(torch.equal(a, b) for a, b in zip(again[2], dfeats))
    assert torch.equal(head.loss(feats, props, gts, sample_inds=pick)["loss_bbox"], losses["loss_bbox"])
    enc = make_roi(c, reg_target="encoded").loss(feats, props, gts, sample_inds=pick)      # mmdet's target
    for k in ("loss_cls", "loss_bbox", "acc"):
        held("%s_head_encoded_%s" % (name, k), enc[k].reshape(1), np.asarray(r["loss"]["encoded"][k]).reshape(1), np.asarray(y["loss"]["encoded"][k]).reshape(1))
    # the reference's own call: bbox_loss on given scores and deltas
    res = head.bbox_loss(HC.K, s, s["rois"], dict(cls_score=dev(r["cls"].astype(F32)), bbox_pred=dev(r["reg"].astype(F32))))
    q64, q32 = roi_restated(r["cls"].astype(F32), r["reg"].astype(F32), HC.K, lists, "reference", F64), roi_restated(r["cls"].astype(F32), r["reg"].astype(F32), HC.K, lists, "reference", F32)
    for k in ("loss_cls", "loss_bbox", "acc"):
        held("%s_bbox_loss_%s" % (name, k), res["loss_bbox"][k].reshape(1), np.asarray(q64[k]).reshape(1), np.asarray(q32[k]).reshape(1))


def test_roi_head_with_predictors_passed_per_call():
    """the reference's form: a head without num_classes, fc_cls and fc_reg owned by the caller"""
    name = "full"
    c, feats, gts, props, ref, _ = roi_setup(name)
    pick = picks(ref["roi"]["samples"])
    own, bare = make_roi(c), make_roi(c, num_classes=None)
    assert sorted(bare.state_dict()) == ["bbox_head.shared_fcs.%d.%s" % (i, k) for i in (0, 1) for k in ("bias", "weight")]
    fc_cls, fc_reg = torch.nn.Linear(HC.FC_OUT, HC.K + 1).cuda(), torch.nn.Linear(HC.FC_OUT, 4 * HC.K).cuda()
    with torch.no_grad():
        for m, k in ((fc_cls, "fc_cls"), (fc_reg, "fc_reg")):
            m.weight.copy_(torch.as_tensor(c["roi"][k + ".weight"]))
            m.bias.copy_(torch.as_tensor(c["roi"][k + ".bias"]))
    a = own.loss_and_grads(feats, props, gts, sample_inds=pick)
    b = bare.loss_and_grads(feats, props, gts, num_classes=HC.K, fc_cls=fc_cls, fc_reg=fc_reg, sample_inds=pick)
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[1]["bbox_head.fc_reg.weight"], b[1]["fc_reg.weight"]) and torch.equal(a[1]["bbox_head.shared_fcs.0.weight"], b[1]["bbox_head.shared_fcs.0.weight"])
    with pytest.raises(ValueError):
        bare.loss_and_grads(feats, props, gts, sample_inds=pick)
    x_cls, x_reg = bare.bbox_head(own.train_bbox_forward(feats, own.gen_sampling_results(props, gts, sample_inds=pick))[0])
    assert tuple(x_cls.shape) == (HC.BATCH * HC.ROI_NUM, HC.FC_OUT) and x_cls is x_reg
    da, db = own.predict(feats, props, HC.METAS), bare.predict(feats, props, HC.METAS, num_classes=HC.K, fc_cls=fc_cls, fc_reg=fc_reg)
    assert all(torch.equal(p.keep, q.keep) and torch.equal(p.bboxes, q.bboxes) for p, q in zip(da, db))


def check_dets(tag, got, ref, yard):
    for b, r in enumerate(got):
        keep, bx, sc, lab, _, _ = ref[b]
        assert r.keep.tolist() == keep.tolist() and r.labels.tolist() == lab.tolist()      # exact, in output order
        held("%s_boxes_%d" % (tag, b), r.bboxes, bx, yard[b][1])
        held("%s_scores_%d" % (tag, b), r.scores, sc, yard[b][2])


@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_roi_head_predict(name):
    c, feats, gts, props, ref, y32 = roi_setup(name)
    head = make_roi(c)
    check_dets(name + "_det", head.predict(feats, props, HC.METAS), ref["dets"]["plain"], y32["dets"]["plain"])
    check_dets(name + "_det_rescale", head.predict(feats, props, HC.METAS, rescale=True), ref["dets"]["rescale"], y32["dets"]["rescale"])
    check_dets(name + "_det_top", head.predict(feats, props, HC.METAS, rcnn_test_cfg=HC.RCNN_TOP), ref["dets"]["top"], y32["dets"]["top"])
    # the reference's calls one by one
    proposals, rois = head.test_bbox_generate_roi(props)
    res = head._bbox_forward(feats, rois)
    held(name + "_cls_score", res["cls_score"], ref["tcls"], y32["tcls"])
    held(name + "_bbox_pred", res["bbox_pred"], ref["treg"], y32["treg"])
    check_dets(name + "_predict_bbox", head.predict_bbox(HC.METAS, res, proposals, rois, HC.RCNN, HC.K, False), ref["dets"]["plain"], y32["dets"]["plain"])
    raw = head.predict_bbox(HC.METAS, res, proposals, rois, None, HC.K, False)
    n0 = int((ref["test_rois"][:, 0] == 0).sum())
    assert tuple(raw[0].bboxes.shape) == (n0, 4 * HC.K) and tuple(raw[0].scores.shape) == (n0, HC.K + 1)
    held(name + "_raw_scores", raw[0].scores[:, :HC.K], ref["dets"]["plain"][0][4], y32["dets"]["plain"][0][4])
    import roi_ref
    held(name + "_raw_scores_with_background", raw[0].scores, roi_ref.softmax(ref["tcls"][:n0]), roi_ref.softmax(y32["tcls"][:n0], F32))
    held(name + "_raw_boxes", raw[0].bboxes.reshape(n0, HC.K, 4), ref["dets"]["plain"][0][5], y32["dets"]["plain"][0][5])
    none = head.predict(feats, [NS(bboxes=torch.zeros(0, 4, device="cuda")) for _ in props], HC.METAS)      # R = 0: empty results, the library untouched
    assert all(len(r.scores) == 0 and tuple(r.bboxes.shape) == (0, 4) for r in none)


def bf16_round(a):
    return torch.as_tensor(np.asarray(a, F32)).to(torch.bfloat16).to(torch.float32).numpy()


def test_roi_layers_bf16_vs_cpu(precision="bf16"):
    """the layers alone in 'bf16' against the same layers in numpy on the CPU with the operands rounded where the engine keeps bf16, forward and
    backward through the padded predictors.  (In 'fp32' the layers are held on the cases' own inputs: cls_score and bbox_pred in
    test_roi_head_predict, the parameter and map gradients in test_roi_head_loss_and_grads.)"""
    import roi_ref
    c = HC.case("full")
    rng = np.random.default_rng(8)
    Rn, K = 70, HC.K
    x = rng.normal(0, 1, (Rn, HC.C, HC.P, HC.P)).astype(F32)
    dcls, dreg = rng.normal(0, 0.1, (Rn, K + 1)).astype(F32), rng.normal(0, 0.1, (Rn, 4 * K)).astype(F32)
    rnd = bf16_round
    tc, tr, tctx = roi_ref.fc_forward(x.reshape(Rn, -1), c["roi"], F64, rnd)
    tG, tdx = roi_ref.fc_backward(dcls, dreg, tctx)
    yc, yr, yctx = roi_ref.fc_forward(x.reshape(Rn, -1), c["roi"], F32, rnd)
    yG, ydx = roi_ref.fc_backward(dcls, dreg, yctx, F32)
    head = make_roi(c, precision).bbox_head
    cls, reg = head(dev(x))
    tag = "hbox_layers_%s_" % precision
    held(tag + "cls", cls, tc, yc)
    held(tag + "reg", reg, tr, yr)
    eng, out, ctx, K = head.forward_rows(head.rows_of(dev(x)))
    c0 = head.reg_col(K)
    dout = torch.zeros_like(out)
    dout[:, :K + 1], dout[:, c0:c0 + 4 * K] = torch.as_tensor(dcls).cuda(), torch.as_tensor(dreg).cuda()
    G = {n: torch.zeros_like(p) for n, p in head.named_parameters()}
    dx = head.backward_rows(eng, dout, ctx, G, head.predictors()[3], K)
    bm = lambda a: np.ascontiguousarray(np.transpose(a.reshape(Rn, HC.C, -1), (0, 2, 1))).reshape(Rn, -1)      # noqa: E731
    held(tag + "dx", dx, bm(tdx), bm(ydx))
    for k in G:
        held(tag + k, G[k], tG[k], yG[k])


def test_coder_class():
    p, g = coder_inputs(65, 3)
    coder = DeltaXYWHBBoxCoder(target_means=HC.ROI_MEANS, target_stds=HC.ROI_STDS)
    d64, d32 = both(R.encode, p, g, HC.ROI_MEANS, HC.ROI_STDS)
    held("coder_encode", coder.encode(dev(p), dev(g)), d64, d32)
    deltas = (d64 * 1.5).astype(F32)
    r64, r32 = both(R.decode, p, deltas, HC.ROI_MEANS, HC.ROI_STDS, max_shape=(40, 48))
    held("coder_decode", coder.decode(dev(p), dev(deltas), max_shape=(40, 48)), r64, r32)
    r64, r32 = both(R.decode, p, deltas, HC.ROI_MEANS, HC.ROI_STDS)
    held("coder_decode_unclipped", coder.decode(dev(p), dev(deltas)), r64, r32)
    assert tuple(coder.encode(torch.zeros(0, 4, device="cuda"), torch.zeros(0, 4, device="cuda")).shape) == (0, 4) and coder.encode_size == 4


# ------------------------------------------------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_end_to_end_training(name):
    """RPNHead.loss_and_predict -> HBoxRoIHead.gen_sampling_results -> HBoxRoIHead.loss_and_grads -> the positives -> MaskRoIHead.loss_and_grads,
    every stage fed by the stage before it on the device, against the chained restatement"""
    c, feats, gts = inputs(name)
    ref, y32 = HC.reference(name), HC.yardstick(name)
    rpn, roi = make_rpn(c), make_roi(c)
    mask, conv_logits = make_mask(c)
    losses, proposals = rpn.loss_and_predict(feats, gts, HC.METAS, sample_inds=picks(ref["rpn"]["samples"]))
    held(name + "_e2e_loss_rpn_cls", torch.stack(losses["loss_rpn_cls"]), ref["rpn"]["loss_cls"], y32["rpn"]["loss_cls"])
    held(name + "_e2e_loss_rpn_bbox", torch.stack(losses["loss_rpn_bbox"]), ref["rpn"]["loss_bbox"], y32["rpn"]["loss_bbox"])
    check_proposals(name + "_e2e", proposals, ref["rpn"]["props"], y32["rpn"]["props"])
    pick = picks(ref["roi"]["samples"])
    rl, G, dfeats, s = roi.loss_and_grads(feats, proposals, gts, sample_inds=pick, return_samples=True)
    r, y = ref["roi"], y32["roi"]
    assert s["n_pos"].tolist() == r["lists"]["n_pos"].tolist() and s["sample_gt"].tolist() == r["lists"]["sample_gt"].tolist()
    for k in ("loss_cls", "loss_bbox", "acc"):
        held("%s_e2e_%s" % (name, k), rl[k].reshape(1), np.asarray(r["loss"]["reference"][k]).reshape(1), np.asarray(y["loss"]["reference"][k]).reshape(1))
    for l in range(len(HC.ROI_STRIDES)):
        held("%s_e2e_dfeat_%d" % (name, l), dfeats[l], r["dfeats"][l], y["dfeats"][l])
    m, my = ref["mask"]["train"], y32["mask"]["train"]
    ml, mG, mdf, aux = mask.loss_and_grads(feats, s["pos"], dict(bitmaps=dev(c["bitmaps"]) if len(c["bitmaps"]) else torch.zeros(0, 64, 64, dtype=torch.uint8, device="cuda")),
                                           conv_logits, return_aux=True)
    held(name + "_e2e_loss_mask", ml["loss_mask"].reshape(1), np.asarray(m["loss_mask"]).reshape(1), np.asarray(my["loss_mask"]).reshape(1))
    first = (np.arange(HC.BATCH)[:, None] * HC.ROI_NUM + np.arange(MC.S)[None]).reshape(-1)      # the restatement's slots: the first S of every image
    assert np.array_equal(aux["mask_targets"].cpu().numpy()[first], m["targets"])      # exact
    for l in range(len(MC.STRIDES)):
        held("%s_e2e_mask_dfeat_%d" % (name, l), mdf[l], m["grads"]["feats.%d" % l], my["grads"]["feats.%d" % l])
    for k in c["mask"]:
        held("%s_e2e_d_%s" % (name, k), mG["mask_head." + k], m["grads"]["mask_head." + k], my["grads"]["mask_head." + k])


@pytest.mark.parametrize("name", list(HC.SHAPES))
def test_end_to_end_test_time(name):
    """RPNHead.predict -> HBoxRoIHead.predict_bbox -> MaskRoIHead.predict, against the chained restatement"""
    c, feats, gts = inputs(name)
    ref, y32 = HC.reference(name), HC.yardstick(name)
    rpn, roi = make_rpn(c), make_roi(c)
    mask, conv_logits = make_mask(c)
    proposals = rpn.predict(feats, HC.METAS)
    check_proposals(name + "_t2t", proposals, ref["rpn"]["props"], y32["rpn"]["props"])
    check_dets(name + "_t2t_det", roi.predict(feats, proposals, HC.METAS), ref["dets"]["plain"], y32["dets"]["plain"])
    props, rois = roi.test_bbox_generate_roi(proposals)      # the reference's calls: the list predict_bbox returns is what MaskRoIHead.predict takes
    dets = roi.predict_bbox(HC.METAS, roi._bbox_forward(feats, rois), props, rois, HC.RCNN_TOP, HC.K, False)
    check_dets(name + "_t2t_top", dets, ref["dets"]["top"], y32["dets"]["top"])
    again = roi.predict(feats, proposals, HC.METAS, rcnn_test_cfg=HC.RCNN_TOP)
    assert all(torch.equal(a.keep, d.keep) and torch.equal(a.bboxes, d.bboxes) for a, d in zip(again, dets))
    metas = [dict(img_shape=HC.IMG, ori_shape=HC.IMG, scale_factor=(1.0, 1.0))] * HC.BATCH
    out = mask.predict(feats, dets, metas, conv_logits)
    for b, res in enumerate(out):
        want = ref["mask"]["pasted"][b][1]
        assert res.masks.dtype == torch.bool and np.array_equal(res.masks.cpu().numpy(), want) and want.any() and not want.all()      # exact
