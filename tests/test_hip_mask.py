"""GPU: the mask branch (mtp_amd/csrc/mask_head.hip and what stands on it) on the inputs of tests/mask_cases.py, against fixture f25 (the reference's own
mask_head.py / roi_head.py in float64, tests/golden/make_mask_branch.py) and, where f25 has nothing (aligned=False, a fixed sampling ratio,
caller-given levels, the thinned-out rows of f25), against tests/mask_ref.py in float64, which tests/test_mask_host.py holds to f25.
Every output is a poisoned, guarded buffer of a guard.Arena, every input is frozen, the wrappers' own workspaces come from the arena too.

Targets and pasted masks are compared bit for bit: mask_cases' seeds keep every float64 value 1e-4 away from its threshold.  Every float bound is
4 x the error of the float32 CPU restatement against float64 on the same inputs (floor 1e-6), computed here; both numbers are in the message."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import guard
import mask_cases as MC
import mask_ref as MR
from conftest import record_parity
from mtp_amd import MODELS, ops

pytestmark = pytest.mark.gpu
CASES = list(MC.SHAPES)
ARENA = None
SCALES = [1.0 / s for s in MC.STRIDES]
R = MC.BATCH * MC.S


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


@pytest.fixture(scope="module")
def f25(golden):
    return golden("f25_mask_branch.npz")


def padded(f25, name, key, dtype=np.float64):
    """a per-positive record of f25 (the reference has no padding) in the fixed-slot layout, zeros on the padding"""
    a, use = f25[name + "." + key], MC.in_use(MC.case(name))
    out = np.zeros((len(use),) + a.shape[1:], dtype)
    out[use] = a
    return out


def thin(a, name, f25):
    """what f25 records of mask_feats / mask_preds: everything for 'base', every step-th row and column of the other cases"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    step = int(f25["step"])
    return a if name == "base" else np.ascontiguousarray(a[..., ::step, ::step])


def dev(a):
    """an op INPUT on the device, frozen"""
    return ARENA.frozen(ARENA.like(torch.as_tensor(np.ascontiguousarray(a))))


def err_of(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a.astype(np.float64) - ref).max()) if ref.size else 0.0


def held(tag, out, ref64, ref32):
    """4 x the float32 CPU error of the restatement against float64, floor 1e-6"""
    ref64 = np.asarray(ref64, np.float64)
    err, e32 = err_of(out, ref64), err_of(np.asarray(ref32), ref64)
    record_parity("mask", tag, err)
    record_parity("mask", "mask_ref_f32_cpu_" + tag, e32)
    print("%s: err %.3e, float32 restatement %.3e" % (tag, err, e32))
    assert tuple(out.shape) == ref64.shape and err < max(4 * e32, 1e-6), (tag, err, e32)


def bin_major(x):
    """(R, C, P, P) -> the kernels' (R, P P, C)"""
    return np.ascontiguousarray(np.transpose(x.reshape(x.shape[0], x.shape[1], -1), (0, 2, 1)))


def rows_of(maps, ld):
    """NCHW maps -> per level (N H W, ld) rows whose first C columns are the channels, the rest zeros"""
    out = []
    for m in maps:
        N, Cc, H, W = m.shape
        r = np.zeros((N * H * W, ld), np.float32)
        r[:, :Cc] = np.transpose(m, (0, 2, 3, 1)).reshape(-1, Cc)
        out.append(r)
    return out


def nchw_of(rows, shape):
    N, Cc, H, W = shape
    return np.transpose(rows[:, :Cc].reshape(N, H, W, Cc), (0, 3, 1, 2))


def align_inputs(name):
    c = MC.case(name)
    sizes = [f.shape[2:] for f in c["feats"]]
    return c, sizes, dev(c["rois"]), dev(c["n_pos"])


GIVEN = (np.arange(R) % len(MC.STRIDES)).astype(np.int32)      # caller-given levels: the large boxes land on the fine maps (adaptive grid 3)


# ------------------------------------------------------------------------------------------------------------------- 1. RoIAlign forward
@pytest.mark.parametrize("sampling", [0, 2])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_roi_align_forward(name, aligned, sampling, f25):
    c, sizes, rois, n_pos = align_inputs(name)
    Cc, ld = c["C"], c["C"] + 4
    maps = [ops.rpn_map_rows(dev(r), H, W) for r, (H, W) in zip(rows_of(c["feats"], ld), sizes)]
    use = MC.in_use(c)
    for given in (None, GIVEN):
        out, lv = ARENA.empty(R, MC.OUT * MC.OUT, Cc), ARENA.empty(R, dtype=torch.int32)
        ops.roi_align_fwd(maps, sizes, SCALES, Cc, MC.BATCH, rois, MC.OUT, sampling, aligned, MC.FINEST, roi_levels=None if given is None else dev(given),
                          valid=n_pos, out=out, levels_out=lv)
        ARENA.check_written(out)
        ARENA.check_written(lv)
        ref64, lv64 = MR.roi_align(c["feats"], c["rois"], MC.STRIDES, MC.OUT, sampling, aligned, MC.FINEST, levels=given, in_use=use)
        ref32, _ = MR.roi_align(c["feats"], c["rois"], MC.STRIDES, MC.OUT, sampling, aligned, MC.FINEST, levels=given, in_use=use, ft=np.float32)
        assert np.array_equal(lv.cpu().numpy(), np.where(use, lv64, -1)), "levels"
        assert not out[torch.as_tensor(~use)].any(), "a slot that is not in use is zero"
        held("roi_align_fwd_%s_a%d_s%d_%s" % (name, aligned, sampling, "map" if given is None else "given"), out, bin_major(ref64), bin_major(ref32))
        if aligned and sampling == 0 and given is None:      # what the reference runs: its own record
            assert np.array_equal(lv.cpu().numpy()[use], f25[name + ".levels"]), "levels against f25"
            nchw = out.cpu().numpy().transpose(0, 2, 1).reshape(R, Cc, MC.OUT, MC.OUT)
            held("roi_align_fwd_%s_f25" % name, torch.as_tensor(thin(nchw, name, f25)), thin(padded(f25, name, "mask_feats"), "base", f25), thin(ref32, name, f25))


def test_roi_align_forward_without_valid_uses_every_slot():
    c, sizes, rois, _ = align_inputs("one_empty")
    maps = [ops.rpn_map_nchw(dev(f)) for f in c["feats"]]
    out = ARENA.empty(R, MC.OUT * MC.OUT, c["C"])
    ops.roi_align_fwd(maps, sizes, SCALES, c["C"], MC.BATCH, rois, MC.OUT, 0, True, MC.FINEST, out=out)
    ref64, _ = MR.roi_align(c["feats"], c["rois"], MC.STRIDES, MC.OUT, 0, True, MC.FINEST)
    ref32, _ = MR.roi_align(c["feats"], c["rois"], MC.STRIDES, MC.OUT, 0, True, MC.FINEST, ft=np.float32)
    held("roi_align_fwd_nchw_all_slots", out, bin_major(ref64), bin_major(ref32))


# ------------------------------------------------------------------------------------------------------------------- 2. RoIAlign backward
@pytest.mark.parametrize("sampling", [0, 2])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_roi_align_backward(name, aligned, sampling):
    c, sizes, rois, n_pos = align_inputs(name)
    Cc, ld = c["C"], c["C"] + 4
    shapes = [f.shape for f in c["feats"]]
    use = MC.in_use(c)
    rng = np.random.default_rng(7)
    d = rng.standard_normal((R, Cc, MC.OUT, MC.OUT)).astype(np.float32)
    dout = dev(bin_major(d))
    for given in (None, GIVEN):
        lv = None if given is None else dev(given)
        args = (sizes, SCALES, Cc, MC.BATCH, rois, MC.OUT, sampling, aligned, MC.FINEST)
        ref64 = MR.roi_align_bwd(d, shapes, c["rois"], MC.STRIDES, MC.OUT, sampling, aligned, MC.FINEST, levels=given, in_use=use)
        ref32 = MR.roi_align_bwd(d, shapes, c["rois"], MC.STRIDES, MC.OUT, sampling, aligned, MC.FINEST, levels=given, in_use=use, ft=np.float32)
        runs = []
        for _ in range(2):      # overwrite: every pixel of every level is stored, and two runs give the same bits
            wide = [ARENA.wide(s[0] * s[2] * s[3], ld) for s in shapes]
            cols = [ARENA.cols(w, 0, Cc) for w in wide]
            ops.roi_align_bwd(dout, [ops.rpn_map_rows(w, H, W) for w, (H, W) in zip(wide, sizes)], *args, roi_levels=lv, valid=n_pos)
            for col in cols:
                ARENA.check_written(col.contiguous())
            runs.append([col.clone() for col in cols])
        tag = "roi_align_bwd_%s_a%d_s%d_%s" % (name, aligned, sampling, "map" if given is None else "given")
        for i, (a, b) in enumerate(zip(*runs)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ in bits, level %d" % i
            held("%s_l%d" % (tag, i), torch.as_tensor(nchw_of(a.cpu().numpy(), shapes[i])), ref64[i], ref32[i])
        # accumulate: added to what is there
        base = [rng.standard_normal(s).astype(np.float32) for s in shapes]
        acc = [ARENA.like(torch.as_tensor(b)) for b in base]
        ops.roi_align_bwd(dout, [ops.rpn_map_nchw(a) for a in acc], *args, roi_levels=lv, valid=n_pos, accumulate=True)
        for i, a in enumerate(acc):
            held("%s_acc_l%d" % (tag, i), a, base[i].astype(np.float64) + ref64[i], base[i] + ref32[i])


# ------------------------------------------------------------------------------------------------------------------- 2b. grids beyond the dense walk
def big_counts():
    """per RoI of MC.BIG_ROIS (grid_y, grid_x) in float64: the adaptive grid at its caller-given level, cut at 2^24"""
    out = []
    for roi, l in zip(MC.BIG_ROIS, MC.BIG_LEVELS):
        s = 1.0 / MC.STRIDES[l]
        out.append((MR.axis(roi[2], roi[4], s, MC.OUT, 0, True, np.float64)[2], MR.axis(roi[1], roi[3], s, MC.OUT, 0, True, np.float64)[2]))
    return np.array(out, np.float64)


def test_roi_align_beyond_the_dense_grid():
    """grids of 11, 54, thousands and beyond the cut at 2^24 per axis: the kernels walk only the stretch of a bin's grid that can fall inside the
    map; mask_ref finds the live samples by bisection on the coordinate (held to a scan of every sample in tests/test_mask_host.py).  count makes
    the averages of the largest boxes tiny, so every comparison is made twice: as it is, and with each RoI scaled by its count (the bound scales
    with it); the backward gets a dout scaled the same way, so that every RoI weighs in the gradient."""
    c = MC.case("base")
    Cc, n = c["C"], len(MC.BIG_ROIS)
    sizes, shapes = [f.shape[2:] for f in c["feats"]], [f.shape for f in c["feats"]]
    grids = big_counts()
    assert grids.min(1).max() == MR.MAX_GRID and (grids.max(1) >= 11).all() and (grids.min(1) >= 10).sum() >= 6, "beyond the dense walk (8), on both axes for most"
    cnt = grids[:, 0] * grids[:, 1]
    rois, lv = dev(MC.BIG_ROIS), dev(MC.BIG_LEVELS)
    maps = [ops.rpn_map_nchw(dev(f)) for f in c["feats"]]
    out = ARENA.empty(n, MC.OUT * MC.OUT, Cc)
    ops.roi_align_fwd(maps, sizes, SCALES, Cc, MC.BATCH, rois, MC.OUT, 0, True, MC.FINEST, roi_levels=lv, out=out)
    ARENA.check_written(out)
    ref64, _ = MR.roi_align(c["feats"], MC.BIG_ROIS, MC.STRIDES, MC.OUT, 0, True, MC.FINEST, levels=MC.BIG_LEVELS)
    ref32, _ = MR.roi_align(c["feats"], MC.BIG_ROIS, MC.STRIDES, MC.OUT, 0, True, MC.FINEST, levels=MC.BIG_LEVELS, ft=np.float32)
    assert np.abs(ref64[:5]).reshape(5, -1).max(1).min() > 1e-7 and np.abs(ref64[0]).max() > 0.05, "the boxes do sample their maps"
    held("big_grid_fwd", out, bin_major(ref64), bin_major(ref32))
    for r in range(n):      # per RoI and times its count, so that each has a bound of its own size
        held("big_grid_fwd_%d_times_count" % r, out[r].double().cpu() * cnt[r], bin_major(ref64)[r] * cnt[r], bin_major(ref32)[r].astype(np.float64) * cnt[r])
    rng = np.random.default_rng(5)
    # the backward: the moderate grids alone (a bound of their own), then all RoIs; dout times the count where float32 still places the samples
    for tag, pick, scale in (("moderate", [0, 1, 4], cnt[[0, 1, 4]]), ("all", list(range(n)), np.where(np.arange(n) < 5, cnt, 1.0))):
        d = (rng.standard_normal((len(pick), Cc, MC.OUT, MC.OUT)) * scale[:, None, None, None]).astype(np.float32)
        rr, ll = np.ascontiguousarray(MC.BIG_ROIS[pick]), np.ascontiguousarray(MC.BIG_LEVELS[pick])
        dout, rois_p, lv_p = dev(bin_major(d)), dev(rr), dev(ll)
        g64 = MR.roi_align_bwd(d, shapes, rr, MC.STRIDES, MC.OUT, 0, True, MC.FINEST, levels=ll)
        g32 = MR.roi_align_bwd(d, shapes, rr, MC.STRIDES, MC.OUT, 0, True, MC.FINEST, levels=ll, ft=np.float32)
        runs = []
        for _ in range(2):
            grads = [ARENA.empty(*s) for s in shapes]
            ops.roi_align_bwd(dout, [ops.rpn_map_nchw(g) for g in grads], sizes, SCALES, Cc, MC.BATCH, rois_p, MC.OUT, 0, True, MC.FINEST, roi_levels=lv_p)
            for g in grads:
                ARENA.check_written(g)
            runs.append(grads)
        for l, (x, y) in enumerate(zip(*runs)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "two runs differ in bits, level %d" % l
            held("big_grid_bwd_%s_l%d" % (tag, l), x, g64[l], g32[l])
        assert np.abs(g64[0]).max() > 0.1 and np.abs(g64[1]).max() > 0.1 and not g64[2].any()


def test_mask_targets_beyond_the_dense_grid():
    """280 x 300 bitmaps sampled at 28 x 28: grids of 10 and 11 per axis in the target kernel"""
    bm, boxes = MC.big_bitmaps(), MC.BIG_BOXES
    n, rows = len(boxes), np.array([[0, 1, 0, 1]], np.int64)
    assert int(np.ceil(np.clip(boxes[:, 2], 0, 300) - np.clip(boxes[:, 0], 0, 300)).max() / MC.M) >= 10
    z = (np.random.default_rng(13).standard_normal((n, 1, MC.M, MC.M)) * 2.0).astype(np.float32)
    got = dict(loss=ARENA.empty(1), targets=ARENA.empty(n, MC.M, MC.M, dtype=torch.uint8), slot_loss=ARENA.empty(n), target_avg=ARENA.empty(n, MC.M, MC.M))
    dl = ARENA.empty(n, 1, MC.M, MC.M)
    ops.mask_loss(dev(z), dev(boxes), None, dev(rows), dev(np.array([n], np.int64)), dev(bm), loss_weight=MC.LOSS_WEIGHT, dlogits=dl, out=got)
    refs = []
    for ft in (np.float64, np.float32):
        avg, tg = MR.mask_targets(boxes, rows[0], bm, MC.M, ft=ft)
        refs.append((avg, tg) + MR.mask_loss(z, tg, np.zeros(n, np.int64), n, MC.LOSS_WEIGHT, ft))
    (a64, t64, l64, s64, d64), (a32, _, l32, s32, d32) = refs
    grids = [MR.axis(np.clip(b[0], 0, 300), np.clip(b[2], 0, 300), 1.0, MC.M, 0, True, np.float64)[2] for b in boxes]
    assert min(grids) >= 10 and float(np.abs(a64 - 0.5).min()) > MC.MARGIN and 0.2 < t64.mean() < 0.8
    assert np.array_equal(got["targets"].cpu().numpy(), t64), "targets, bit for bit"
    held("big_grid_avg", got["target_avg"], a64, a32)
    held("big_grid_loss", got["loss"], np.asarray([l64]), np.asarray([l32]))
    held("big_grid_slot", got["slot_loss"], s64, s32)
    held("big_grid_dlogits", dl, d64, d32)


# ------------------------------------------------------------------------------------------------------------------- 3. targets and loss
def loss_inputs(c, K=MC.K, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, K, MC.M, MC.M)) * 2.0).astype(np.float32)


def loss_refs(c, z, n_pos, labels):
    use = (np.arange(MC.S)[None, :] < n_pos[:, None]).reshape(-1)
    out = []
    for ft in (np.float64, np.float32):
        avg, tg = np.zeros((R, MC.M, MC.M), ft), np.zeros((R, MC.M, MC.M), np.uint8)
        if use.any():
            avg[use], tg[use] = MR.mask_targets(c["boxes"][use], c["sample_gt"].reshape(-1)[use], c["bitmaps"], MC.M, ft=ft)
        loss, slot, d = MR.mask_loss(z, tg, np.where(use, labels, -1), int(n_pos.sum()), MC.LOSS_WEIGHT, ft)
        out.append(dict(avg=avg, targets=tg, loss=np.asarray([loss]), slot=slot, d=d))
    return use, out[0], out[1]


def check_loss(tag, c, z, n_pos_np, labels_np, got, dl, f25=None):
    use, r64, r32 = loss_refs(c, z, n_pos_np, labels_np)
    if f25 is not None:      # the reference's own targets and the averages behind them
        assert np.array_equal(got["targets"].cpu().numpy(), padded(f25, c["name"], "targets", np.uint8)), "targets against f25, bit for bit"
        held(tag + "_avg_f25", got["target_avg"], padded(f25, c["name"], "target_avg"), r32["avg"])
    for k in ("loss", "slot_loss", "target_avg"):
        ARENA.check_written(got[k])
    ARENA.check_written(dl)
    margin = float(np.abs(r64["avg"][use] - 0.5).min()) if use.any() else 1.0
    assert margin > MC.MARGIN, "the case keeps its target averages away from the threshold"
    assert np.array_equal(got["targets"].cpu().numpy(), r64["targets"]), "targets, bit for bit"
    held(tag + "_avg", got["target_avg"], r64["avg"], r32["avg"])
    held(tag + "_loss", got["loss"], r64["loss"], r32["loss"])
    held(tag + "_slot", got["slot_loss"], r64["slot"], r32["slot"])
    held(tag + "_dlogits", dl, r64["d"], r32["d"])
    pad = torch.as_tensor(~use)
    assert not dl[pad].any() and not got["slot_loss"][pad].any() and not got["targets"][pad].any(), "padding slots are zero"
    other = np.ones((R, z.shape[1]), bool)
    other[np.arange(R), labels_np] = False
    assert not dl[torch.as_tensor(other)].any(), "the other class channels are zero"
    if not use.any():
        assert float(got["loss"][0]) == 0.0 and not dl.any(), "no positive: exactly 0 and all-zero gradients"


@pytest.mark.parametrize("name", CASES)
def test_mask_targets_and_loss(name, f25):
    c = MC.case(name)
    z = loss_inputs(c)
    logits, boxes, labels, sample_gt, bitmaps = dev(z), dev(c["boxes"]), dev(c["labels"]), dev(c["sample_gt"]), dev(c["bitmaps"])
    n_pos = ARENA.like(torch.as_tensor(c["n_pos"]))
    got = dict(loss=ARENA.empty(1), targets=ARENA.empty(R, MC.M, MC.M, dtype=torch.uint8), slot_loss=ARENA.empty(R), target_avg=ARENA.empty(R, MC.M, MC.M))
    dl = ARENA.empty(R, MC.K, MC.M, MC.M)
    ops.mask_loss(logits, boxes, labels, sample_gt, n_pos, bitmaps, loss_weight=MC.LOSS_WEIGHT, dlogits=dl, out=got)
    check_loss("mask_loss_" + name, c, z, c["n_pos"], c["labels"], got, dl, f25)
    # the counts change ON THE DEVICE, nothing is reallocated or passed again: the second call sees them, so nothing was read on the host
    fewer = np.maximum(c["n_pos"] - 2, 0)
    n_pos.copy_(torch.clamp(n_pos - 2, min=0))
    ops.mask_loss(logits, boxes, labels, sample_gt, n_pos, bitmaps, loss_weight=MC.LOSS_WEIGHT, dlogits=dl, out=got)
    check_loss("mask_loss_%s_fewer" % name, c, z, fewer, c["labels"], got, dl)


def test_mask_loss_labels_beyond_num_classes_are_padding():
    """the head hands the loss its GEMM output padded to 8 channels: the labels name the first num_classes of them; a slot whose label lies beyond
    is padding (no loss, no gradient), and still counts in n_pos_total, which is the sum of n_pos"""
    c = MC.case("base")
    Kc = 8
    z = loss_inputs(c, K=Kc, seed=14)
    labels = c["labels"].copy()
    use = MC.in_use(c)
    labels[np.nonzero(use)[0][1]] = MC.K      # a channel that exists in the tensor and not among the classes
    labels[np.nonzero(use)[0][4]] = Kc + 3
    got = dict(loss=ARENA.empty(1), targets=ARENA.empty(R, MC.M, MC.M, dtype=torch.uint8), slot_loss=ARENA.empty(R), target_avg=ARENA.empty(R, MC.M, MC.M))
    dl = ARENA.empty(R, Kc, MC.M, MC.M)
    ops.mask_loss(dev(z), dev(c["boxes"]), dev(labels), dev(c["sample_gt"]), dev(c["n_pos"]), dev(c["bitmaps"]), loss_weight=MC.LOSS_WEIGHT, dlogits=dl, out=got,
                  num_classes=MC.K)
    live = use & (labels < MC.K)
    assert live.sum() == use.sum() - 2
    refs = []
    for ft in (np.float64, np.float32):
        tg = np.zeros((R, MC.M, MC.M), np.uint8)
        tg[live] = MR.mask_targets(c["boxes"][live], c["sample_gt"].reshape(-1)[live], c["bitmaps"], MC.M, ft=ft)[1]
        refs.append((tg,) + MR.mask_loss(z, tg, np.where(live, labels, -1), int(use.sum()), MC.LOSS_WEIGHT, ft))
    (t64, l64, s64, d64), (_, l32, s32, d32) = refs
    ARENA.check_written(dl)
    assert np.array_equal(got["targets"].cpu().numpy(), t64)
    held("mask_loss_beyond_classes_loss", got["loss"], np.asarray([l64]), np.asarray([l32]))
    held("mask_loss_beyond_classes_dlogits", dl, d64, d32)
    assert not dl[torch.as_tensor(~live)].any() and not dl[:, MC.K:].any() and not got["slot_loss"][torch.as_tensor(~live)].any()


def test_mask_loss_class_agnostic_and_image_sizes():
    """labels=None: channel 0 of a one-channel head; img_hw: the boxes are clipped to each image's own (h, w) inside the padded bitmaps"""
    c = MC.case("base")
    z = loss_inputs(c, K=1, seed=12)
    hw = np.array([[52, 60], [61, 47]], np.int64)
    got = dict(loss=ARENA.empty(1), targets=ARENA.empty(R, MC.M, MC.M, dtype=torch.uint8), slot_loss=ARENA.empty(R), target_avg=ARENA.empty(R, MC.M, MC.M))
    dl = ARENA.empty(R, 1, MC.M, MC.M)
    ops.mask_loss(dev(z), dev(c["boxes"]), None, dev(c["sample_gt"]), dev(c["n_pos"]), dev(c["bitmaps"]), img_hw=dev(hw), loss_weight=0.5, dlogits=dl, out=got)
    use = MC.in_use(c)
    per_slot = np.repeat(hw, MC.S, 0)[use]
    refs = []
    for ft in (np.float64, np.float32):
        avg, tg = np.zeros((R, MC.M, MC.M), ft), np.zeros((R, MC.M, MC.M), np.uint8)
        avg[use], tg[use] = MR.mask_targets(c["boxes"][use], c["sample_gt"].reshape(-1)[use], c["bitmaps"], MC.M, img_hw=per_slot, ft=ft)
        refs.append((avg, tg) + MR.mask_loss(z, tg, np.where(use, 0, -1), int(use.sum()), 0.5, ft))
    (a64, t64, l64, s64, d64), (a32, _, l32, s32, d32) = refs
    assert float(np.abs(a64[use] - 0.5).min()) > MC.MARGIN, "these sizes keep the target averages away from the threshold"
    assert np.array_equal(got["targets"].cpu().numpy(), t64), "targets, bit for bit"
    held("mask_loss_agnostic_avg", got["target_avg"], a64, a32)
    held("mask_loss_agnostic_loss", got["loss"], np.asarray([l64]), np.asarray([l32]))
    held("mask_loss_agnostic_slot", got["slot_loss"], s64, s32)
    held("mask_loss_agnostic_dlogits", dl, d64, d32)


# ------------------------------------------------------------------------------------------------------------------- 4. paste
@pytest.mark.parametrize("threshold", [MC.THR, -1.0])
@pytest.mark.parametrize("name", ["base", "odd"])
def test_mask_paste(name, threshold, f25):
    c = MC.case(name)
    p = c["paste"]
    logits, labels = dev(p["logits"]), dev(p["labels"])
    for rescale, boxes, h, w in MC.paste_frames(c):
        N = len(boxes)
        out, vals = ARENA.empty(N, h, w, dtype=torch.uint8), ARENA.empty(N, h, w)
        masks = ops.mask_paste(logits, labels, dev(boxes), h, w, threshold, out=out, values=vals)
        v64, m64 = MR.paste(p["logits"], p["labels"], boxes, h, w, threshold)
        v32, _ = MR.paste(p["logits"], p["labels"], boxes, h, w, threshold, ft=np.float32)
        tag = "mask_paste_%s_%s_%s" % (name, "rescale" if rescale else "scaled", "bool" if threshold >= 0 else "u8")
        assert not np.isnan(v64).any()
        held(tag, vals, v64, v32)
        kind = "bool" if threshold >= 0 else "u8"
        recorded = f25["%s.paste.%s.%s.masks" % (name, "rescale" if rescale else "scaled", kind)]
        if threshold >= 0:
            assert float(np.abs(v64 - threshold).min()) > MC.MARGIN
            assert masks.dtype == torch.bool and np.array_equal(masks.cpu().numpy(), m64), "masks, bit for bit"
            assert np.array_equal(masks.cpu().numpy(), recorded.astype(bool)), "masks against f25, bit for bit"
            assert 0.02 < m64.mean() < 0.9
        else:
            assert masks.dtype == torch.uint8 and int(np.abs(masks.cpu().numpy().astype(np.int64) - m64.astype(np.int64)).max()) <= 1, "uint8 within one count"
            assert int(np.abs(masks.cpu().numpy().astype(np.int64) - recorded.astype(np.int64)).max()) <= 1, "uint8 against f25 within one count"


def test_mask_paste_label_without_a_channel_is_an_empty_mask():
    """also at mask_thr_binary = 0, where a value of 0 would pass the threshold"""
    c = MC.case("base")
    p = c["paste"]
    _, boxes, h, w = MC.paste_frames(c)[0]
    labels = p["labels"].copy()
    labels[1], labels[4] = MC.K, -1
    for thr in (0.0, -1.0):
        out, vals = ARENA.empty(len(boxes), h, w, dtype=torch.uint8), ARENA.empty(len(boxes), h, w)
        ops.mask_paste(dev(p["logits"]), dev(labels), dev(boxes), h, w, thr, out=out, values=vals)
        ARENA.check_written(vals)
        assert not out[1].any() and not out[4].any() and not vals[1].any() and not vals[4].any()
        _, want = MR.paste(p["logits"], p["labels"], boxes, h, w, thr)
        keep = [0, 2, 3, 5]
        if thr >= 0:
            assert np.array_equal(out.cpu().numpy()[keep].astype(bool), want[keep]) and want[keep].all(), "a sigmoid is >= 0 everywhere"
        else:
            assert int(np.abs(out.cpu().numpy()[keep].astype(np.int64) - want[keep].astype(np.int64)).max()) <= 1


def test_mask_paste_class_agnostic_raw_values():
    """labels=None takes channel 0; activate=False pastes the values as they are (the reference's activate_map)"""
    c = MC.case("base")
    p = c["paste"]
    _, boxes, h, w = MC.paste_frames(c)[0]
    z = MR.sigmoid(p["logits"][:, :1], np.float32)
    out, vals = ARENA.empty(len(boxes), h, w, dtype=torch.uint8), ARENA.empty(len(boxes), h, w)
    ops.mask_paste(dev(z), None, dev(boxes), h, w, MC.THR, activate=False, out=out, values=vals)
    v64, _ = MR.paste(z, None, boxes, h, w, MC.THR, activate=False)
    v32, _ = MR.paste(z, None, boxes, h, w, MC.THR, activate=False, ft=np.float32)
    held("mask_paste_raw", vals, v64, v32)
    off = np.abs(v64 - MC.THR) > MC.MARGIN
    assert np.array_equal(out.cpu().numpy().astype(bool)[off], (v64 >= MC.THR)[off])


# ------------------------------------------------------------------------------------------------------------------- 5. the head, end to end
def make_head(c, precision="fp32", slots=MC.S):
    """MTP_IS_StandardRoIHead as mask_rcnn.py configures it, at the cases' sizes, with the case's weights; and the data set's conv_logits"""
    head = MODELS.build(dict(
        type="MTP_IS_StandardRoIHead",
        mask_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=MC.OUT, sampling_ratio=0), out_channels=c["C"],
                                featmap_strides=list(MC.STRIDES), finest_scale=MC.FINEST),
        mask_head=dict(type="MTP_IS_FCNMaskHead", num_convs=MC.NUM_CONVS, in_channels=c["C"], conv_out_channels=MC.CONV,
                       loss_mask=dict(type="CrossEntropyLoss", use_mask=True, loss_weight=MC.LOSS_WEIGHT), precision=precision),
        train_cfg=dict(mask_size=MC.M, sampler=dict(type="RandomSampler", num=4 * slots, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True), pos_weight=-1,
                       debug=False),
        test_cfg=dict(mask_thr_binary=MC.THR))).cuda()
    head.load_state_dict({"mask_head." + k: torch.as_tensor(v) for k, v in c["weights"].items()})
    conv_logits = torch.nn.Conv2d(MC.CONV, MC.K, 1).cuda()
    with torch.no_grad():
        conv_logits.weight.copy_(torch.as_tensor(c["conv_logits"]["weight"]))
        conv_logits.bias.copy_(torch.as_tensor(c["conv_logits"]["bias"]))
    return head, conv_logits


def slot_samples(c):
    return dict(boxes=dev(c["boxes"]), sample_gt=dev(c["sample_gt"]), labels=dev(c["labels"]), n_pos=dev(c["n_pos"]))


def list_samples(c):
    """the reference's form: per image pos_priors, pos_assigned_gt_inds, pos_gt_labels; and the bitmaps per image"""
    samples = [NS(pos_priors=dev(p["boxes"].reshape(-1, 4)), pos_assigned_gt_inds=dev(p["gt"]), pos_gt_labels=dev(p["labels"])) for p in c["pos"]]
    masks = [dev(c["bitmaps"][a:b]) for a, b in zip(c["gt_start"][:-1], c["gt_start"][1:])]
    return samples, masks


@pytest.fixture(scope="module")
def runs():
    """the CPU runs of every case, once: float64 (the reference), float32 and float32 with bf16 operands (the yardsticks)"""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            c = MC.case(name)
            cache[(name, kind)] = MC.run(c) if kind == "f64" else MC.run(c, np.float32, torch.bfloat16 if kind == "bf16" else None)
        return cache[(name, kind)]
    return get


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_loss_and_grads(name, precision, runs, f25):
    c = MC.case(name)
    r64, y = runs(name, "f64"), runs(name, "f32" if precision == "fp32" else "bf16")
    head, conv_logits = make_head(c, precision)
    feats = [dev(f) for f in c["feats"]]
    samples, gt = slot_samples(c), dict(bitmaps=dev(c["bitmaps"]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # nothing between the samples and the loss waits on the host
    try:
        losses, G, dfeats, aux = head.loss_and_grads(feats, samples, gt, conv_logits, return_aux=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    use = MC.in_use(c)
    tag = "%s_%s_" % (name, precision)
    y32 = runs(name, "f32")
    assert np.array_equal(aux["levels"].cpu().numpy(), np.where(use, r64["levels"], -1)) and np.array_equal(aux["levels"].cpu().numpy()[use], f25[name + ".levels"])
    held(tag + "mask_feats", aux["mask_feats"], bin_major(r64["mask_feats"]), bin_major(y32["mask_feats"]))
    feats_nchw = aux["mask_feats"].cpu().numpy().transpose(0, 2, 1).reshape(R, c["C"], MC.OUT, MC.OUT)
    held(tag + "mask_feats_f25", torch.as_tensor(thin(feats_nchw, name, f25)), thin(padded(f25, name, "mask_feats"), "base", f25), thin(y32["mask_feats"], name, f25))
    held(tag + "mask_preds", aux["mask_preds"], r64["mask_preds"], y["mask_preds"])
    held(tag + "mask_preds_f25", torch.as_tensor(thin(aux["mask_preds"], name, f25)[use]), f25[name + ".mask_preds"], thin(y["mask_preds"], name, f25)[use])
    assert np.array_equal(aux["mask_targets"].cpu().numpy(), padded(f25, name, "targets", np.uint8)), "targets against f25, bit for bit"
    held(tag + "loss_mask", losses["loss_mask"].reshape(1), f25[name + ".loss_mask"].reshape(1), y["loss_mask"].reshape(1))
    assert sorted(G) == sorted(k[len(name) + 6:] for k in f25 if k.startswith(name + ".grad.")) and all(p.grad is None for p in head.parameters())
    for k, g in G.items():
        held(tag + "d_" + k, g, f25["%s.grad.%s" % (name, k)], y["grads"][k])
    for l, d in enumerate(dfeats):
        held(tag + "dfeat_%d" % l, d, f25["%s.level%d.dfeat" % (name, l)], y["grads"]["feats.%d" % l])
    if not use.any():
        assert float(losses["loss_mask"]) == 0.0 and not any(g.any() for g in G.values()) and not any(d.any() for d in dfeats), "no positive: exactly zero"
    # two calls: the same bits (the bias gradients are the GEMMs' column-sum by-product, which the GEMM launchers add with atomics in every head:
    # they are held to the bound above, not to bit identity)
    again = head.loss_and_grads(feats, samples, gt, conv_logits)
    assert torch.equal(again[0]["loss_mask"], losses["loss_mask"]) and all(torch.equal(a, b) for a, b in zip(again[2], dfeats))
    assert torch.equal(head.loss(feats, samples, gt, conv_logits)["loss_mask"], losses["loss_mask"])
    # the reference's form of the samples is laid into the same slots: the same bits
    ls, lm = list_samples(c)
    other = head.loss_and_grads(feats, ls, lm, conv_logits, return_aux=True)
    assert torch.equal(other[0]["loss_mask"], losses["loss_mask"]) and all(torch.equal(a, b) for a, b in zip(other[2], dfeats))
    assert torch.equal(other[3]["mask_targets"], aux["mask_targets"]) and torch.equal(other[3]["mask_preds"], aux["mask_preds"])
    assert all(torch.equal(other[1][k], G[k]) for k in G if k.endswith("weight"))


def test_head_in_chunks(runs, f25):
    """more slots than head_chunk: the layers run chunk after chunk, the loss over the whole batch"""
    name = "base"
    c = MC.case(name)
    y = runs(name, "f32")
    head, conv_logits = make_head(c)
    head.head_chunk = 6      # 16 slots: 6 + 6 + 4, the cut inside image 0 and inside image 1
    feats = [dev(f) for f in c["feats"]]
    losses, G, dfeats, aux = head.loss_and_grads(feats, slot_samples(c), dict(bitmaps=dev(c["bitmaps"])), conv_logits, return_aux=True)
    assert np.array_equal(aux["mask_targets"].cpu().numpy(), padded(f25, name, "targets", np.uint8))
    held("chunks_mask_preds", aux["mask_preds"][torch.as_tensor(MC.in_use(c))], f25[name + ".mask_preds"], y["mask_preds"][MC.in_use(c)])
    held("chunks_loss_mask", losses["loss_mask"].reshape(1), f25[name + ".loss_mask"].reshape(1), y["loss_mask"].reshape(1))
    for k, g in G.items():
        held("chunks_d_" + k, g, f25["%s.grad.%s" % (name, k)], y["grads"][k])
    for l, d in enumerate(dfeats):
        held("chunks_dfeat_%d" % l, d, f25["%s.level%d.dfeat" % (name, l)], y["grads"]["feats.%d" % l])
    assert torch.equal(head.loss(feats, slot_samples(c), dict(bitmaps=dev(c["bitmaps"])), conv_logits)["loss_mask"], losses["loss_mask"])
    mh = head.mask_head
    x = dev(np.random.default_rng(2).normal(0, 1, (7, c["C"], MC.OUT, MC.OUT)).astype(np.float32))
    whole = mh(x, conv_logits)
    mh.forward_chunk = 3
    assert torch.equal(mh(x, conv_logits), whole), "the chunks run the same per-row GEMMs: the same bits"


def test_reference_calls_train_and_test():
    """models.py:284-305 call by call: train_mask_forward -> mask_head -> conv_logits -> mask_loss; test_mask_generate_rois -> test_mask_roi_feats ->
    mask_head -> conv_logits -> predict_mask"""
    c = MC.case("base")
    head, conv_logits = make_head(c)
    feats = [dev(f) for f in c["feats"]]
    ls, lm = list_samples(c)
    use = MC.in_use(c)
    r64, r32 = MC.run(c), MC.run(c, np.float32)
    mask_feats = head.train_mask_forward(feats, ls, None)
    held("calls_mask_feats", mask_feats, r64["mask_feats"][use], r32["mask_feats"][use])
    x_mask = head.mask_head(mask_feats)
    assert tuple(x_mask.shape) == (int(use.sum()), MC.CONV, MC.M, MC.M)
    mask_preds = head.mask_head(mask_feats, conv_logits)
    held("calls_mask_preds", mask_preds, r64["mask_preds"][use], r32["mask_preds"][use])
    gts = [NS(masks=m) for m in lm]
    res = head.mask_loss(dict(mask_preds=mask_preds, mask_feats=mask_feats), ls, gts)
    held("calls_loss_mask", res["loss_mask"]["loss_mask"].reshape(1), r64["loss_mask"].reshape(1), r32["loss_mask"].reshape(1))
    assert np.array_equal(res["mask_targets"].cpu().numpy(), r64["targets"][use])
    assert torch.equal(head.mask_head.get_targets(ls, gts, head.train_cfg), res["mask_targets"])
    # test time: the paste of the case, through the head (rescale on and off)
    p = c["paste"]
    for rescale, boxes, h, w in MC.paste_frames(c):
        results = [NS(bboxes=dev(p["boxes"][:4]), labels=dev(p["labels"][:4])), NS(bboxes=dev(p["boxes"][4:]), labels=dev(p["labels"][4:]))]
        metas = [dict(ori_shape=MC.PASTE_HW, scale_factor=MC.PASTE_SCALE)] * 2
        out = head.predict_mask(metas, results, dict(mask_preds=dev(p["logits"])), rescale=rescale)
        _, m64 = MR.paste(p["logits"], p["labels"], boxes, h, w, MC.THR)
        got = torch.cat([r.masks for r in out])
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), m64), "masks, bit for bit"
        if rescale:
            held("calls_rescaled_boxes", torch.cat([r.bboxes for r in out]), boxes.astype(np.float64), boxes)
    rois = head.test_mask_generate_rois([NS(bboxes=dev(c["pos"][b]["boxes"].reshape(-1, 4))) for b in range(MC.BATCH)])
    assert tuple(rois.shape) == (int(use.sum()), 5)
    held("calls_test_feats", head.test_mask_roi_feats(feats, rois), r64["mask_feats"][use], r32["mask_feats"][use])
    empty = head.predict(feats, [NS(bboxes=torch.zeros(0, 4, device="cuda"), labels=torch.zeros(0, dtype=torch.int64, device="cuda"))] * 2,
                         [dict(ori_shape=MC.PASTE_HW, scale_factor=(1.0, 1.0))] * 2, conv_logits)
    assert all(tuple(r.masks.shape) == (0,) + MC.PASTE_HW for r in empty), "N = 0: empty masks, the library untouched"


def test_roi_align_module_autograd():
    """mtp_amd.ops_roi.RoIAlign: one level with a graph, the gradient by the gather kernel; R = 0 without the library"""
    from mtp_amd.ops_roi import RoIAlign
    c = MC.case("base")
    use = MC.in_use(c)
    x = dev(c["feats"][0]).clone().requires_grad_(True)
    layer = RoIAlign(MC.OUT, 1.0 / MC.STRIDES[0], 0)
    rois = c["rois"][use]
    out = layer(x, dev(rois))
    d = np.random.default_rng(3).standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(dev(d))
    lv = np.zeros(len(rois), np.int64)
    shapes = [f.shape for f in c["feats"]]
    f64, f32 = [(MR.roi_align(c["feats"], rois, MC.STRIDES, MC.OUT, 0, True, MC.FINEST, levels=lv, ft=ft)[0],
                 MR.roi_align_bwd(d, shapes, rois, MC.STRIDES, MC.OUT, 0, True, MC.FINEST, levels=lv, ft=ft)[0]) for ft in (np.float64, np.float32)]
    held("module_fwd", out.detach(), f64[0], f32[0])
    held("module_bwd", x.grad, f64[1], f32[1])
    y = layer(x, torch.zeros(0, 5, device="cuda"))
    assert tuple(y.shape) == (0, c["C"], MC.OUT, MC.OUT)


def test_weight_image_cache_and_invalidate_weights():
    """the GEMM images of the convs and of the deconvolution are kept per weight version: a write through torch is seen; a write that goes round
    the version counter (as the project's optimizer and broadcast kernels do) is seen after invalidate_weights()"""
    c = MC.case("base")
    head, conv_logits = make_head(c)
    mh = head.mask_head
    x = dev(np.random.default_rng(1).normal(0, 1, (5, c["C"], MC.OUT, MC.OUT)).astype(np.float32))
    first = mh(x, conv_logits).clone()
    assert torch.equal(mh(x, conv_logits), first) and mh._images["packs"] == 1, "the second run reuses the images"
    with torch.no_grad():
        mh.upsample.weight.mul_(0.5)      # through torch: the version counter moves
    second = mh(x, conv_logits).clone()
    assert not torch.equal(second, first) and mh._images["packs"] == 2
    mh.upsample.weight.data.mul_(2.0)      # round the counter: the cached image is still the halved one
    assert torch.equal(mh(x, conv_logits), second)
    head.invalidate_weights()
    assert torch.equal(mh(x, conv_logits), first)      # halving and doubling are exact: the first weights again
