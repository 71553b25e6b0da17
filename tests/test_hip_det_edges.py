"""GPU: the kernels of the two detection heads (csrc/roi_head.hip, csrc/rpn.hip) at the seams and cut-offs their feature tests stay away from, every
buffer out of a guard.Arena (poisoned outputs, guards on both sides, frozen inputs, the wrappers' own workspaces included).  The references are
tests/roi_ref.py, tests/rpn_ref.py and tests/box_ref.py in float64; the inputs are those of tests/det_edge_cases.py, whose conditions
tests/test_det_edges_host.py asserts.
  1. RoIAlignRotated forward and backward: C = 64, 65, 130 (gridDim.y of the gather 1, 2 with one live lane, 3); eight (out_size, sample_num), three
     of them on the limit of 1024 points, both `clockwise`; dyadic RoIs whose samples lie exactly on -1, H, W and H - 1, bit for bit; maps one pixel
     high or wide; slots that are not RoIs; thousands of entries in one pixel; R = N = C = 1.
  2. ops.roi_loss and ops.roi_predict called directly: S = 1 .. 600 (a second chunk of the sample list from 257 on) and R = 1 .. 1000 (a second
     workgroup from 257 on), K = 1 .. 80, padded leading dimensions; the device-side clamps; the softmax regimes of test_hip_cls_ops.py; the SmoothL1
     kinks, exact; refusals that launch nothing.
  3. ops.rpn_loss at S = 255, 256, 257, 600 and with out-of-range entries; ops.rpn_proposals with a level that keeps nothing, a level kept whole,
     A = 1 and 9, one level, keep indices out of range.
Exact cases are compared with torch.equal.  Every other bound is `held`: 4 x the error of the float32 CPU restatement against float64 (floor 1e-6),
computed here; both numbers are recorded in the group det_edges."""
import numpy as np
import pytest
import torch

import det_edge_cases as D
import guard
import roi_cases as RC
import roi_ref as R
import rpn_cases as PC
from det_edge_cases import held
from mtp_amd import _lib, ops

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
ARENA = None


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


def all_poison(t):
    view, pat = guard.poison_of(t.dtype)
    return bool((t.contiguous().view(view) == pat).all())


def f32_of(a):
    return torch.as_tensor(np.asarray(a, F64).astype(F32)).cuda()


# ------------------------------------------------------------------------------------------------------------------- 1. RoIAlignRotated
def align_fwd(maps, rois, strides, P, S, cw, levels=None, layout="nchw"):
    """-> out (R, P P, C), levels_out (R)"""
    sizes, (N, Cc), Rn = [m.shape[2:] for m in maps], maps[0].shape[:2], len(rois)
    if layout == "nchw":
        tm = [ops.rpn_map_nchw(dev(m)) for m in maps]
    else:
        tm = [ops.rpn_map_rows(dev(r), H, W) for r, (H, W) in zip(D.rows_of(maps, Cc + 4), sizes)]
    used = ARENA.empty(Rn, dtype=torch.int32)
    out = ops.roi_align_rotated_fwd(tm, sizes, [1.0 / s for s in strides], Cc, N, dev(rois), out_size=P, sample_num=S, clockwise=cw, finest_scale=D.FINEST,
                                    roi_levels=None if levels is None else dev(np.asarray(levels, np.int32)), out=ARENA.empty(Rn, P * P, Cc), levels_out=used)
    return out, used


def align_bwd(dout, shapes, rois, strides, P, S, cw, levels=None, layout="nchw", base=None):
    """-> the gradient buffers: NCHW (zeroed, or holding `base` and accumulated into), or (N H W, C + 4) rows"""
    sizes, (N, Cc) = [s[2:] for s in shapes], shapes[0][:2]
    if layout == "nchw":
        bufs = [ARENA.zeros(*s) for s in shapes] if base is None else [ARENA.like(torch.as_tensor(b)) for b in base]
        tm = [ops.rpn_map_nchw(b) for b in bufs]
    else:
        bufs = [ARENA.zeros(N * H * W, Cc + 4) for H, W in sizes]
        tm = [ops.rpn_map_rows(b, H, W) for b, (H, W) in zip(bufs, sizes)]
    ops.roi_align_rotated_bwd(dev(D.bin_major(dout)), tm, sizes, [1.0 / s for s in strides], Cc, N, dev(rois), out_size=P, sample_num=S, clockwise=cw,
                              finest_scale=D.FINEST, roi_levels=None if levels is None else dev(np.asarray(levels, np.int32)), accumulate=base is not None)
    return bufs


def align_refs(maps, rois, strides, P, S, cw, dout, levels=None, valid=None):
    """(forward float64, float32, backward float64, float32) of the references"""
    shapes = [m.shape for m in maps]
    kw = dict(levels=levels, valid=valid)
    return (D.bin_major(R.roi_align(maps, rois, strides, P, S, cw, D.FINEST, **kw)), D.bin_major(R.roi_align(maps, rois, strides, P, S, cw, D.FINEST, dtype=F32, **kw)),
            D.roi_align_bwd(dout, shapes, rois, strides, P, S, cw, D.FINEST, **kw), D.roi_align_bwd(dout, shapes, rois, strides, P, S, cw, D.FINEST, dtype=F32, **kw))


def dout_of(rois, Cc, P, seed):
    return np.random.default_rng(seed).normal(0, 1, (len(rois), Cc, P, P)).astype(F32)


def check_bwd(tag, g, b64, b32):
    for l in range(len(g)):
        held("%s_bwd_%d" % (tag, l), g[l], b64[l], b32[l])
        assert not g[l].cpu().numpy()[b64[l] == 0].any()      # exactly zero off the touched pixels


@pytest.mark.parametrize("channels", D.WIDE_C)
def test_align_wide_channels(channels):
    maps, rois = D.wide_case(channels)
    P, S, cw, st = RC.P, RC.S, RC.CLOCKWISE, D.STRIDES
    shapes, dout = [m.shape for m in maps], dout_of(rois, channels, RC.P, 7)
    f64, f32, b64, b32 = align_refs(maps, rois, st, P, S, cw, dout)
    a, used = align_fwd(maps, rois, st, P, S, cw)
    b, _ = align_fwd(maps, rois, st, P, S, cw, layout="rows")
    held("wide_fwd_%d" % channels, a, f64, f32)
    assert torch.equal(a, b) and used.tolist() == R.map_levels(rois, 4, D.FINEST).tolist()      # row strides: the same bits
    g = align_bwd(dout, shapes, rois, st, P, S, cw)
    check_bwd("wide_%d" % channels, g, b64, b32)
    assert all((r != 0).any() for r in b64)
    again = align_bwd(dout, shapes, rois, st, P, S, cw)
    assert all(torch.equal(x, y) for x, y in zip(again, g))      # two calls: the same bits
    base = [np.random.default_rng(8 + l).normal(0, 1, s).astype(F32) for l, s in enumerate(shapes)]
    acc = align_bwd(dout, shapes, rois, st, P, S, cw, base=base)
    for x, bl, gl, r in zip(acc, base, g, b64):      # accumulate adds, and leaves what it does not touch
        assert torch.equal(x, torch.as_tensor(bl).cuda() + gl) and np.array_equal(x.cpu().numpy()[r == 0], bl[r == 0])
    rows = align_bwd(dout, shapes, rois, st, P, S, cw, layout="rows")
    for r, gl, (N, Cc, H, W) in zip(rows, g, shapes):      # row strides: the same bits, the padding columns untouched
        assert torch.equal(r[:, :Cc].reshape(N, H, W, Cc).permute(0, 3, 1, 2), gl) and not r[:, Cc:].any()


@pytest.mark.parametrize("P,S,cw", D.GEOMS)
def test_align_geometry(P, S, cw):
    maps, rois = D.geom_case(P, S, cw)
    dout = dout_of(rois, D.GEOM_C, P, 9)
    f64, f32, b64, b32 = align_refs(maps, rois, D.STRIDES, P, S, cw, dout)
    tag = "geom_%d_%d_%s" % (P, S, "cw" if cw else "ccw")
    a, used = align_fwd(maps, rois, D.STRIDES, P, S, cw)
    held(tag + "_fwd", a, f64, f32)
    assert used.tolist() == R.map_levels(rois, 4, D.FINEST).tolist() and not f64[7].any() and np.abs(f64).max() > 0.5
    check_bwd(tag, align_bwd(dout, [m.shape for m in maps], rois, D.STRIDES, P, S, cw), b64, b32)


@pytest.mark.parametrize("P,S", D.GEOM_REFUSED)
def test_align_refuses_more_points_than_the_limit(P, S):
    maps, rois = D.geom_case(7, 3, True)
    sizes, scales = [m.shape[2:] for m in maps], [1.0 / s for s in D.STRIDES]
    out, used = ARENA.empty(len(rois), P * P, D.GEOM_C), ARENA.empty(len(rois), dtype=torch.int32)
    tm = [ops.rpn_map_nchw(dev(m)) for m in maps]
    with pytest.raises(ValueError):
        ops.roi_align_rotated_fwd(tm, sizes, scales, D.GEOM_C, D.BATCH, dev(rois), out_size=P, sample_num=S, clockwise=True, out=out, levels_out=used)
    grads = [ARENA.empty(*m.shape) for m in maps]
    with pytest.raises(ValueError):
        ops.roi_align_rotated_bwd(dev(np.zeros((len(rois), P * P, D.GEOM_C), F32)), [ops.rpn_map_nchw(g) for g in grads], sizes, scales, D.GEOM_C, D.BATCH,
                                  dev(rois), out_size=P, sample_num=S, clockwise=True)
    torch.cuda.synchronize()
    assert all_poison(out) and all_poison(used) and all(all_poison(g) for g in grads)      # nothing was launched


@pytest.mark.parametrize("cw", [True, False])
def test_align_exact_cutoffs(cw):
    """samples exactly on -1, on H and W, on integer pixels and on H - 1: inclusive cut-offs, bit for bit (the host test shows that the expected
    values change when either comparison is made exclusive)"""
    maps, rois, dout = D.exact_case()
    P, S, st = D.EXACT_P, D.EXACT_S, (D.EXACT_STRIDE,)
    f64 = D.bin_major(R.roi_align(maps, rois, st, P, S, cw, D.FINEST))
    b64 = D.roi_align_bwd(dout, [maps[0].shape], rois, st, P, S, cw, D.FINEST)[0]
    for layout in ("nchw", "rows"):
        a, used = align_fwd(maps, rois, st, P, S, cw, layout=layout)
        assert torch.equal(a, f32_of(f64)) and not used.any()
    g = align_bwd(dout, [maps[0].shape], rois, st, P, S, cw)[0]
    assert torch.equal(g, f32_of(b64)) and b64.any()


def test_align_one_pixel_maps():
    rois, lv = D.pixel_case()
    maps = D.pixel_maps()
    dout = dout_of(rois, D.PIXEL_C, D.PIXEL_P, 10)
    f64, f32, b64, b32 = align_refs(maps, rois, D.PIXEL_STRIDES, D.PIXEL_P, D.PIXEL_S, True, dout, levels=lv)
    a, used = align_fwd(maps, rois, D.PIXEL_STRIDES, D.PIXEL_P, D.PIXEL_S, True, levels=lv)
    held("pixel_fwd", a, f64, f32)
    assert used.tolist() == lv.tolist()
    check_bwd("pixel", align_bwd(dout, [m.shape for m in maps], rois, D.PIXEL_STRIDES, D.PIXEL_P, D.PIXEL_S, True, levels=lv), b64, b32)


def test_align_slots_that_are_not_rois():
    """an image index outside the batch (or NaN): zero output, levels_out -1, no gradient written anywhere.  A valid image with NaN sizes: level 0,
    zero output, no gradient.  Zero and negative sizes are numbers: the reference's values.  roi_levels of -3 and 99 clamp to the first and last."""
    maps, rois, P, S = D.geom_maps(), D.SLOT_ROIS, RC.P, RC.S
    shapes, valid, safe = [m.shape for m in maps], D.slot_valid(), D.slot_rois_for_ref()
    dout = dout_of(rois, D.GEOM_C, P, 11)
    f64, f32, b64, b32 = align_refs(maps, safe, D.STRIDES, P, S, True, dout, levels=D.SLOT_LEVELS, valid=valid)
    a, used = align_fwd(maps, rois, D.STRIDES, P, S, True)
    held("slots_fwd", a, f64, f32)
    assert used.tolist() == D.SLOT_LEVELS_OUT.tolist() and not a[D.SLOT_BAD_IMAGE].any() and not a[D.SLOT_NAN_SIZE].any() and all(a[i].any() for i in D.SLOT_FINITE)
    check_bwd("slots", align_bwd(dout, shapes, rois, D.STRIDES, P, S, True), b64, b32)
    # the slots that are not RoIs alone: nothing is written, neither stored into poison nor added to a base
    bad = np.concatenate([rois[D.SLOT_BAD_IMAGE], rois[D.SLOT_NAN_SIZE]])
    grads = [ARENA.empty(*s) for s in shapes]
    ops.roi_align_rotated_bwd(dev(D.bin_major(dout[:len(bad)])), [ops.rpn_map_nchw(g) for g in grads], [s[2:] for s in shapes], [1.0 / s for s in D.STRIDES],
                              D.GEOM_C, D.BATCH, dev(bad), out_size=P, sample_num=S, clockwise=True, accumulate=True)
    torch.cuda.synchronize()
    assert all(all_poison(g) for g in grads)
    z, used = align_fwd(maps, bad, D.STRIDES, P, S, True)
    assert not z.any() and used.tolist() == [-1] * 4 + [0] * 2
    # overridden levels out of range
    want = np.clip(D.SLOT_OVERRIDE, 0, 3)
    o64, o32, _, _ = align_refs(maps, rois[:4], D.STRIDES, P, S, True, dout[:4], levels=want)
    o, used = align_fwd(maps, rois[:4], D.STRIDES, P, S, True, levels=D.SLOT_OVERRIDE)
    held("slots_override", o, o64, o32)
    assert used.tolist() == want.tolist() == [0, 3, 0, 3]


def test_align_hot_pixel():
    """96 sub-pixel RoIs on six pixels: runs of equal keys thousands of entries long, across the workgroups of the gather"""
    rois, dout = D.hot_case()
    rng = np.random.default_rng(12)
    shapes = [(D.BATCH, D.HOT_C, H, W) for H, W in RC.sizes_of((128, 128))]
    b64, b32 = (D.roi_align_bwd(dout, shapes, rois, D.STRIDES, RC.P, RC.S, True, dtype=t) for t in (F64, F32))
    g = align_bwd(dout, shapes, rois, D.STRIDES, RC.P, RC.S, True)
    check_bwd("hot", g, b64, b32)
    assert int((b64[0] != 0).sum()) == 6 * D.HOT_C and not any(b.any() for b in b64[1:])
    again = align_bwd(dout, shapes, rois, D.STRIDES, RC.P, RC.S, True)
    assert all(torch.equal(x, y) for x, y in zip(again, g))
    base = [rng.normal(0, 1, s).astype(F32) for s in shapes]
    acc = align_bwd(dout, shapes, rois, D.STRIDES, RC.P, RC.S, True, base=base)
    assert all(torch.equal(x, torch.as_tensor(bl).cuda() + gl) for x, bl, gl in zip(acc, base, g))


def test_align_smallest():
    maps, roi, dout = D.small_case()
    st = (D.SMALL_STRIDE,)
    f64, f32, b64, b32 = align_refs(maps, roi, st, RC.P, RC.S, True, dout, levels=[0])
    a, used = align_fwd(maps, roi, st, RC.P, RC.S, True)
    held("small_fwd", a, f64, f32)
    assert used.tolist() == [0]
    check_bwd("small", align_bwd(dout, [maps[0].shape], roi, st, RC.P, RC.S, True), b64, b32)


# ------------------------------------------------------------------------------------------------------------------- 2. RoI loss and predict
def run_loss(c, pad, beta=D.BETA, given=None):
    """cls_score and bbox_pred as column slices of one (rows, K + 1 + 5 + pad) buffer, the gradients into a poisoned buffer of the same layout whose
    padding columns the arena checks -> losses (3), dcls, dreg"""
    c = dict(c, **(given or {}))
    K, n = c["K"], c["images"] * c["S"]
    ld = K + 6 + pad
    buf = np.full((n, ld), np.nan, F32)      # a read of a padding column turns a result into NaN
    buf[:, :K + 1], buf[:, K + 1:K + 6] = c["cls"], c["reg"]
    tb = dev(buf)
    grad = ARENA.wide(n, ld)
    dcls, dreg = ARENA.cols(grad, 0, K + 1), ARENA.cols(grad, K + 1, K + 6)
    G = len(c["gts"])
    gts = dev(c["gts"]) if G else torch.zeros(0, 5, device="cuda")
    labels = dev(c["gt_labels"]) if G else torch.zeros(0, dtype=torch.int64, device="cuda")
    losses = ops.roi_loss(tb[:, :K + 1], tb[:, K + 1:K + 6], K, dev(c["rois"]), gts, labels, dev(c["sample_gt"]), dev(c["n_pos"]), dev(c["n_neg"]), D.MEANS, D.STDS,
                          beta, 1.0, 1.0, dcls, dreg, ARENA.empty(3))
    return losses, dcls, dreg


def check_loss(tag, got, r64, r32):
    losses, dcls, dreg = got
    for i, k in enumerate(("loss_cls", "loss_bbox", "acc")):
        held("%s_%s" % (tag, k), losses[i:i + 1], np.asarray(r64[k], F64).reshape(1), np.asarray(r32[k], F32).reshape(1))
    held(tag + "_dcls", dcls, r64["dcls"], r32["dcls"])
    held(tag + "_dreg", dreg, r64["dreg"], r32["dreg"])
    unused = torch.as_tensor(r64["labels"] < 0).cuda()
    nobox = torch.as_tensor(~r64["targets"].any(1)).cuda()      # unused slots and negatives (where a positive's targets are all zero, prior = gt, so are its deltas)
    assert not dcls[unused].any() and not dreg[nobox].any()      # exactly zero


@pytest.mark.parametrize("S,images,K,pad", D.LOSS_CASES)
def test_roi_loss_chunk_seams(S, images, K, pad):
    c = D.loss_case(S, images, K)
    r64, r32 = D.loss_ref(c), D.loss_ref(c, F32)
    got = run_loss(c, pad)
    check_loss("loss_%d_%d_%d" % (S, images, K), got, r64, r32)
    n_neg_rows = int((r64["labels"] == K).sum())
    assert n_neg_rows == int(c["n_neg"].sum()) and int((r64["labels"] >= 0).sum()) == int((c["n_pos"] + c["n_neg"]).sum())
    again = run_loss(c, pad)
    assert all(torch.equal(a, b) for a, b in zip(again, got))      # two calls: the same bits


def test_roi_loss_device_side_clamps():
    c, given, clean = D.clamp_case()
    got = run_loss(c, 3, given=given)
    check_loss("loss_clamped", got, D.loss_ref(c, **clean), D.loss_ref(c, F32, **clean))
    # all images empty: three zeros and zero gradients, nothing divided by zero
    none = dict(n_pos=np.array([0, -3, 0, 0], np.int64), n_neg=np.array([0, 0, -1, 0], np.int64))
    losses, dcls, dreg = run_loss(c, 0, given=none)
    assert losses.tolist() == [0.0, 0.0, 0.0] and not dcls.any() and not dreg.any()
    # no gts at all: every slot in use is a negative, whatever n_pos says
    nogt = dict(gts=np.zeros((0, 5), F32), gt_labels=np.zeros(0, np.int64), n_pos=np.array([3, 0, 0, 5], np.int64), n_neg=np.array([7, 0, 9, 0], np.int64))
    as_neg = dict(nogt, gts=c["gts"], gt_labels=c["gt_labels"], n_pos=np.zeros(4, np.int64), n_neg=np.array([10, 0, 9, 5], np.int64))
    got = run_loss(c, 0, given=nogt)
    check_loss("loss_no_gts", got, D.loss_ref(c, **as_neg), D.loss_ref(c, F32, **as_neg))
    assert float(got[0][1]) == 0 and not got[2].any()


def test_roi_loss_softmax_regimes():
    for name, (c, exact) in D.softmax_cases().items():
        r64, r32 = D.loss_ref(c), D.loss_ref(c, F32)
        got = run_loss(c, 3)
        check_loss("softmax_" + name, got, r64, r32)
        assert float(got[0][2]) == float(r64["acc"])
        if exact:
            assert torch.equal(got[0], f32_of([r64["loss_cls"], r64["loss_bbox"], r64["acc"]])) and torch.equal(got[1], f32_of(r64["dcls"])) and not got[2].any()
    eq = D.softmax_cases()
    assert float(D.loss_ref(eq["equal_label0"][0])["acc"]) == 50.0 and float(D.loss_ref(eq["equal_label3"][0])["acc"]) == 0.0


@pytest.mark.parametrize("beta", D.KINK_BETAS)
def test_roi_loss_smooth_l1_kinks_exact(beta):
    for f in D.KINK_FACTORS:
        lb, dr = D.kink_expected(beta, f)
        losses, dcls, dreg = run_loss(D.kink_case(beta, f), 3, beta=beta)
        assert float(losses[1]) == float(lb) and np.array_equal(dreg.cpu().numpy()[0], dr), (beta, f, float(losses[1]), dreg.tolist())


@pytest.mark.parametrize("Rn,K,pad", D.PREDICT_CASES)
def test_roi_predict(Rn, K, pad):
    c = D.predict_case(Rn, K)
    ld = K + 6 + pad
    buf = np.full((Rn, ld), np.nan, F32)
    buf[:, :K + 1], buf[:, K + 1:K + 6] = c["cls"], c["reg"]
    tb, rois = dev(buf), dev(c["rois"])
    s64, s32 = R.softmax(c["cls"])[:, :K], R.softmax(c["cls"], F32)[:, :K]
    b64, b32 = R.decode(c["rois"], c["reg"], D.MEANS, D.STDS), R.decode(c["rois"], c["reg"], D.MEANS, D.STDS, F32)
    for thr, want in ((D.SCORE_THR, s64 > D.SCORE_THR), (0.0, np.ones_like(s64, bool)), (1.0, np.zeros_like(s64, bool))):
        out = (ARENA.empty(Rn, K), ARENA.empty(Rn, 5), ARENA.empty(Rn, K, dtype=torch.uint8))
        scores, boxes, flags = ops.roi_predict(tb[:, :K + 1], tb[:, K + 1:K + 6], K, rois, D.MEANS, D.STDS, thr, out)
        assert np.array_equal(flags.cpu().numpy(), want.astype(np.uint8))      # exact
    held("predict_scores_%d_%d" % (Rn, K), scores, s64, s32)
    held("predict_boxes_%d_%d" % (Rn, K), boxes, b64, b32)
    assert (boxes[:, 2] >= boxes[:, 3]).all() and (boxes[:, 4] >= -np.pi / 2).all() and (boxes[:, 4] < np.pi / 2).all()


def test_roi_loss_and_predict_refuse_without_a_launch():
    c = D.loss_case(255, 3, 5)
    K, n, S, B = 5, 3 * 255, 255, 3
    ld = K + 6
    buf = np.zeros((n, ld), F32)
    buf[:, :K + 1], buf[:, K + 1:] = c["cls"], c["reg"]
    tb, grad, losses = dev(buf), ARENA.empty(n, ld), ARENA.empty(3)
    cls, reg, dcls, dreg = tb[:, :K + 1], tb[:, K + 1:], grad[:, :K + 1], grad[:, K + 1:]
    t = dict(rois=dev(c["rois"]), gts=dev(c["gts"]), labels=dev(c["gt_labels"]), sg=dev(c["sample_gt"]), n_pos=dev(c["n_pos"]), n_neg=dev(c["n_neg"]))
    args = (K, t["rois"], t["gts"], t["labels"], t["sg"], t["n_pos"], t["n_neg"], D.MEANS)
    with pytest.raises(ValueError):      # a non-positive std
        ops.roi_loss(cls, reg, *args, (0.1, 0.1, 0.0, 0.2, 0.1), 1.0, 1.0, 1.0, dcls, dreg, losses)
    with pytest.raises(ValueError):      # dcls without dreg
        ops.roi_loss(cls, reg, *args, D.STDS, 1.0, 1.0, 1.0, dcls, None, losses)
    with pytest.raises(_lib.MtpHipError):      # beta = 0: the library's own refusal
        ops.roi_loss(cls, reg, *args, D.STDS, 0.0, 1.0, 1.0, dcls, dreg, losses)
    with pytest.raises(TypeError):      # fewer columns than logits
        ops.roi_loss(cls[:, :K], reg, *args, D.STDS, 1.0, 1.0, 1.0, dcls, dreg, losses)
    # the C ABI itself, on the same device buffers
    lib = _lib.load()
    wb = lib.mtp_roi_loss_workspace_bytes(B, S)
    assert wb == B * 1 * 3 * 4
    ws = ARENA.empty(wb // 4)
    m5, s5 = ops._roi_codec(D.MEANS, D.STDS)
    z5 = ops._roi_codec(D.MEANS, (0.1, 0.1, 0.2, 0.2, 0.1))[1]
    z5[3] = -1.0

    def call(ldc=ld, ldr=ld, stds=s5, beta=1.0, pdc=dcls.data_ptr(), pdr=dreg.data_ptr(), bytes_=wb):
        return lib.mtp_roi_loss(cls.data_ptr(), ldc, reg.data_ptr(), ldr, K, t["rois"].data_ptr(), t["gts"].data_ptr(), t["labels"].data_ptr(), D.NUM_G,
                                t["sg"].data_ptr(), t["n_pos"].data_ptr(), t["n_neg"].data_ptr(), B, S, m5, stds, beta, 1.0, 1.0, losses.data_ptr(), pdc, pdr,
                                ws.data_ptr(), bytes_, ops._s())
    assert call(ldc=K) == -1 and call(ldr=4) == -1 and call(stds=z5) == -1 and call(beta=0.0) == -1 and call(pdr=None) == -1 and call(pdc=None) == -1
    assert call(bytes_=wb - 4) == -1      # a workspace one float short
    out = (ARENA.empty(n, K), ARENA.empty(n, 5), ARENA.empty(n, K, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.roi_predict(cls, reg, K, t["rois"], D.MEANS, (0.1, 0.1, 0.2, -0.2, 0.1), 0.05, out)
    with pytest.raises(TypeError):
        ops.roi_predict(cls, reg[:, :4], K, t["rois"], D.MEANS, D.STDS, 0.05, out)

    def pred(ldc=ld, ldr=ld, stds=s5):
        return lib.mtp_roi_predict(cls.data_ptr(), ldc, reg.data_ptr(), ldr, K, t["rois"].data_ptr(), n, m5, stds, 0.05, out[0].data_ptr(), out[1].data_ptr(),
                                   out[2].data_ptr(), ops._s())
    assert pred(ldc=K) == -1 and pred(ldr=4) == -1 and pred(stds=z5) == -1
    torch.cuda.synchronize()
    assert all(all_poison(x) for x in (grad, losses, ws) + out)      # nothing was launched


# ------------------------------------------------------------------------------------------------------------------- 3. the oriented RPN
def rpn_rows_of(maps_cls, maps_reg):
    """the NCHW maps of all levels as one (rows, 24) buffer in the engines' row layout, and each level's first row"""
    blocks, row0, rows = [], [], 0
    for c, r in zip(maps_cls, maps_reg):
        N, A, H, W = c.shape
        m = np.concatenate([c, r, np.zeros((N, 24 - 7 * A, H, W), F32)], 1)
        blocks.append(np.transpose(m, (0, 2, 3, 1)).reshape(N * H * W, 24))
        row0.append(rows)
        rows += N * H * W
    return np.concatenate(blocks), row0


def run_rpn_loss(lists):
    """ops.rpn_loss on rpn_cases' sq128 maps in NCHW strides -> (loss_cls (L), loss_bbox (L), dcls [L], dreg [L]) and the device lists"""
    cls, reg, gts = PC.case(D.RPN_NAME)
    priors, _, sizes = PC.anchors(D.RPN_NAME)
    L = len(sizes)
    mc, mr = [ops.rpn_map_nchw(dev(m)) for m in cls], [ops.rpn_map_nchw(dev(m)) for m in reg]
    dcls, dreg = [ARENA.zeros(*m.shape) for m in cls], [ARENA.zeros(*m.shape) for m in reg]
    t = (dev(priors.astype(F32)), dev(np.concatenate(gts)), dev(lists["samples"]), dev(lists["sample_gt"]), dev(lists["n_pos"]), dev(lists["n_neg"]))
    lc, lb = ops.rpn_loss(mc, mr, sizes, PC.A, *t, PC.MEANS, PC.STDS, PC.BETA, 1.0, 1.0, [ops.rpn_map_nchw(d) for d in dcls], [ops.rpn_map_nchw(d) for d in dreg],
                          ARENA.empty(L), ARENA.empty(L))
    return (lc, lb, dcls, dreg), t


def check_rpn_loss(tag, got, r64, r32):
    lc, lb, dcls, dreg = got
    held(tag + "_loss_cls", lc, r64[0], r32[0])
    held(tag + "_loss_bbox", lb, r64[1], r32[1])
    for l in range(len(dcls)):
        held("%s_dcls_%d" % (tag, l), dcls[l], r64[2][l], r32[2][l])
        held("%s_dreg_%d" % (tag, l), dreg[l], r64[3][l], r32[3][l])
        assert not dcls[l].cpu().numpy()[r64[2][l] == 0].any() and not dreg[l].cpu().numpy()[r64[3][l] == 0].any()      # exactly zero at unsampled anchors


@pytest.mark.parametrize("S", D.RPN_S)
def test_rpn_loss_chunk_seams(S):
    c = D.rpn_seam_case(S)
    got, t = run_rpn_loss(c)
    check_rpn_loss("rpn_%d" % S, got, D.rpn_loss_ref(c), D.rpn_loss_ref(c, F32))
    again, _ = run_rpn_loss(c)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and all(torch.equal(a, b) for a, b in zip(again[2] + again[3], got[2] + got[3]))
    # row strides: one (rows, 24) buffer, the gradient buffer in the same layout; the same bits as NCHW
    cls, reg, _ = PC.case(D.RPN_NAME)
    sizes = PC.anchors(D.RPN_NAME)[2]
    rows, row0 = rpn_rows_of(cls, reg)
    buf, grad = dev(rows), ARENA.zeros(*rows.shape)
    mc = [ops.rpn_map_rows(buf, H, W, 0, r) for (H, W), r in zip(sizes, row0)]
    mr = [ops.rpn_map_rows(buf, H, W, PC.A, r) for (H, W), r in zip(sizes, row0)]
    lc, lb = ops.rpn_loss(mc, mr, sizes, PC.A, *t, PC.MEANS, PC.STDS, PC.BETA, 1.0, 1.0, [(grad,) + m[1:] for m in mc], [(grad,) + m[1:] for m in mr],
                          ARENA.empty(len(sizes)), ARENA.empty(len(sizes)))
    want, _ = rpn_rows_of([d.cpu().numpy() for d in got[2]], [d.cpu().numpy() for d in got[3]])
    assert torch.equal(lc, got[0]) and torch.equal(lb, got[1]) and np.array_equal(grad.cpu().numpy(), want)


def test_rpn_loss_out_of_range_entries():
    """sample indices of -1 and num_priors are skipped (and still counted in avg_factor), a sample_gt of K leaves a positive without a box term,
    n_pos beyond S is S: the reference's values on the cleaned lists"""
    given, clean, avg = D.rpn_bad_case()
    got, _ = run_rpn_loss(given)
    check_rpn_loss("rpn_bad", got, D.rpn_loss_ref(clean, avg_factor=avg), D.rpn_loss_ref(clean, F32, avg_factor=avg))


@pytest.mark.parametrize("name", list(D.PROP_SHAPES))
def test_rpn_proposals(name):
    c = D.prop_case(name)
    A, sizes, counts = c["A"], c["sizes"], c["keep_counts"]
    keep = np.stack([np.concatenate(kb) for kb in c["keep"]]).astype(np.int64)
    T = keep.shape[1]
    per_level = [H * W * A for H, W in sizes]
    ids = np.concatenate([np.full(k, l, np.int64) for l, k in enumerate(counts)])
    given = keep.copy()
    given[0, 1], given[1, T - 1] = -1, per_level[ids[T - 1]]      # a keep index of -1 and one of `count`: zero score, zero boxes, not valid
    bad = np.zeros((D.BATCH, T), bool)
    bad[0, 1] = bad[1, T - 1] = True
    out = (ARENA.empty(D.BATCH, T), ARENA.empty(D.BATCH, T, 5), ARENA.empty(D.BATCH, T, 4), ARENA.empty(D.BATCH, T, dtype=torch.int64),
           ARENA.empty(D.BATCH, T, dtype=torch.uint8))
    scores, rboxes, hboxes, level_ids, valid = ops.rpn_proposals(
        [ops.rpn_map_nchw(dev(m)) for m in c["cls"]], [ops.rpn_map_nchw(dev(m)) for m in c["reg"]], sizes, A, dev(c["priors"].astype(F32)), dev(given), counts,
        PC.MEANS, PC.STDS, D.PROP_MIN_SIZE, out)
    for b in range(D.BATCH):
        r64, r32 = [list(D.prop_ref(c, b, t)) for t in (F64, F32)]
        assert r64[3].tolist() == ids.tolist()
        for r in (r64, r32):
            for i in range(3):
                r[i] = np.where(bad[b].reshape((-1,) + (1,) * (r[i].ndim - 1)), 0, r[i])
        held("prop_%s_scores_%d" % (name, b), scores[b], r64[0], r32[0])
        held("prop_%s_rboxes_%d" % (name, b), rboxes[b], r64[1], r32[1])
        held("prop_%s_hboxes_%d" % (name, b), hboxes[b], r64[2], r32[2])
        want = (r64[1][:, 2] > D.PROP_MIN_SIZE) & (r64[1][:, 3] > D.PROP_MIN_SIZE) & ~bad[b]
        assert level_ids[b].tolist() == ids.tolist() and valid[b].tolist() == want.astype(int).tolist()      # exact
        assert not scores[b][torch.as_tensor(bad[b]).cuda()].any() and not rboxes[b][torch.as_tensor(bad[b]).cuda()].any()
