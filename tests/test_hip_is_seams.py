"""GPU: the instance-segmentation kernels (csrc/mask_head.hip, csrc/hbox_head.hip) at the sizes where their loops take a second trip, on the inputs
of tests/is_seam_cases.py, whose conditions tests/test_is_seams_host.py asserts from the float64 restatements alone.
  1. RoIAlign with 130 RoIs (three trips of the backward's walk, hits in lane 0 and lane 63), C = 1 .. 257 (every register of a lane, a second
     channel chunk), 82 pixels (an image and a level boundary inside a workgroup, idle waves in the last), NCHW and row layout, valid counts,
     accumulate;
  2. out_size 1 .. 32, fixed grids 8, 9 and 64, levels outside [0, n), image indices that name no image;
  3. the mask loss at M M = 1, 4, 256, 289, over 99 slots, with n_pos outside [0, S];
  4. the paste's 0 / 0;
  5. the RPN loss over one to three chunks of sample slots, the RoI loss over more than 64 partial rows, proposals over three workgroups.
Every output is a poisoned, guarded buffer of a guard.Arena, every input is frozen, the wrappers' workspaces come from the arena.  Bits (targets,
masks, levels, flags, gradient signs) are compared exactly; every float with is_seam_cases.held: 4 x the error of the float32 CPU restatement
against float64 (floor 1e-6), both numbers recorded."""
import numpy as np
import pytest
import torch

import guard
import hbox_cases as HC
import is_seam_cases as SC
import mask_cases as MC
import mask_ref as MR
from is_seam_cases import bin_major, held, nchw_of, rows_of
from mtp_amd import ops

pytestmark = pytest.mark.gpu
ARENA = None
F64, F32 = np.float64, np.float32
AL_SIZES = [tuple(s) for s in SC.AL_SIZES]


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


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------- RoIAlign, both directions
def align_fwd(feats, layout, rois, levels, P, sampling, valid=None):
    """-> (out (R, P P, C), levels_out (R)) out of poisoned buffers; layout 'rows': the maps are the first C columns of wider rows"""
    Cc, images, n = feats[0].shape[1], feats[0].shape[0], len(rois)
    if layout == "rows":
        maps = [ops.rpn_map_rows(dev(r), H, W) for r, (H, W) in zip(rows_of(feats, Cc + 3), AL_SIZES)]
    else:
        maps = [ops.rpn_map_nchw(dev(f)) for f in feats]
    out, lv = ARENA.empty(n, P * P, Cc), ARENA.empty(n, dtype=torch.int32)
    ops.roi_align_fwd(maps, AL_SIZES, SC.AL_SCALES, Cc, images, rois, P, sampling, True, SC.AL_FINEST, roi_levels=levels, valid=valid, out=out, levels_out=lv)
    ARENA.check_written(out)
    ARENA.check_written(lv)
    return out, lv


def align_bwd(dout, shapes, layout, rois, levels, P, sampling, valid=None):
    """two runs into fresh poisoned buffers, which must agree in bits -> per level the gradient as an NCHW array.  'rows': the gradient maps are the
    first C columns of wider rows; the arena checks that the other columns keep their poison"""
    Cc, images = shapes[0][1], shapes[0][0]
    runs = []
    for _ in range(2):
        if layout == "rows":
            wide = [ARENA.wide(s[0] * s[2] * s[3], Cc + 3) for s in shapes]
            grads = [ARENA.cols(w, 0, Cc) for w in wide]
            maps = [ops.rpn_map_rows(w, H, W) for w, (H, W) in zip(wide, AL_SIZES)]
        else:
            grads = [ARENA.empty(*s) for s in shapes]
            maps = [ops.rpn_map_nchw(g) for g in grads]
        ops.roi_align_bwd(dout, maps, AL_SIZES, SC.AL_SCALES, Cc, images, rois, P, sampling, True, SC.AL_FINEST, roi_levels=levels, valid=valid)
        for g in grads:
            ARENA.check_written(g.contiguous())
        runs.append([g.clone() for g in grads])
    for l, (a, b) in enumerate(zip(*runs)):
        assert same_bits(a, b), "two runs differ in bits, level %d" % l
    return [nchw_of(g.cpu().numpy(), s) if layout == "rows" else g.cpu().numpy() for g, s in zip(runs[0], shapes)]


@pytest.mark.parametrize("layout", ["nchw", "rows"])
@pytest.mark.parametrize("Cc", SC.AL_C)
def test_roi_align_chunks(Cc, layout):
    c, refs = SC.align_case(), SC.align_refs("all")
    feats = [np.ascontiguousarray(f[:, :Cc]) for f in c["feats"]]
    rois, levels = dev(c["rois"]), dev(c["levels"])
    out, lv = align_fwd(feats, layout, rois, levels, SC.AL_OUT, 0)
    assert np.array_equal(lv.cpu().numpy(), c["levels"]), "levels"
    held("chunks_fwd_c%d_%s" % (Cc, layout), out, bin_major(refs["fwd64"][:, :Cc]), bin_major(refs["fwd32"][:, :Cc]))
    dout = dev(bin_major(c["dout"][:, :Cc]))
    grads = align_bwd(dout, [f.shape for f in feats], layout, rois, levels, SC.AL_OUT, 0)
    for l, g in enumerate(grads):
        held("chunks_bwd_c%d_%s_l%d" % (Cc, layout, l), torch.as_tensor(np.ascontiguousarray(g)), refs["bwd64"][l][:, :Cc], refs["bwd32"][l][:, :Cc])


def test_roi_align_chunks_valid_counts_and_accumulate():
    """C = 65 (two registers of lane 0, one of the others): slots taken out of use by the counts of five groups of 26; and accumulate, which adds
    to what the maps hold"""
    Cc = SC.AL_VALID_C
    c, refs, use = SC.align_case(), SC.align_refs("valid"), SC.align_in_use("valid")
    feats = [np.ascontiguousarray(f[:, :Cc]) for f in c["feats"]]
    shapes = [f.shape for f in feats]
    rois, levels, valid = dev(c["rois"]), dev(c["levels"]), dev(np.asarray(SC.AL_COUNTS, np.int64))
    dout = dev(bin_major(c["dout"][:, :Cc]))
    for layout in ("nchw", "rows"):
        out, lv = align_fwd(feats, layout, rois, levels, SC.AL_OUT, 0, valid=valid)
        assert np.array_equal(lv.cpu().numpy(), np.where(use, c["levels"], -1)), "levels"
        assert not out[torch.as_tensor(~use)].any(), "a slot that is not in use is zero"
        held("chunks_valid_fwd_" + layout, out, bin_major(refs["fwd64"]), bin_major(refs["fwd32"]))
        for l, g in enumerate(align_bwd(dout, shapes, layout, rois, levels, SC.AL_OUT, 0, valid=valid)):
            held("chunks_valid_bwd_%s_l%d" % (layout, l), torch.as_tensor(np.ascontiguousarray(g)), refs["bwd64"][l], refs["bwd32"][l])
    every = SC.align_refs("all")
    rng = np.random.default_rng(9)
    for tag, v, r in (("valid", valid, refs), ("all", None, every)):
        base = [rng.standard_normal(s).astype(F32) for s in shapes]
        acc = [ARENA.like(torch.as_tensor(b)) for b in base]
        ops.roi_align_bwd(dout, [ops.rpn_map_nchw(a) for a in acc], AL_SIZES, SC.AL_SCALES, Cc, SC.AL_IMAGES, rois, SC.AL_OUT, 0, True, SC.AL_FINEST,
                          roi_levels=levels, valid=v, accumulate=True)
        for l, a in enumerate(acc):
            held("chunks_acc_%s_l%d" % (tag, l), a, base[l].astype(F64) + r["bwd64"][l][:, :Cc], base[l] + r["bwd32"][l][:, :Cc])


def run_sizes(tag, rois_np, levels_np, P, sampling, dout_np, want_levels):
    feats = SC.size_feats()
    f64, f32, g64, g32 = SC.size_refs(rois_np, levels_np, P, sampling, dout_np)
    rois, levels = dev(rois_np), dev(levels_np)
    out, lv = align_fwd([np.ascontiguousarray(f) for f in feats], "nchw", rois, levels, P, sampling)
    assert np.array_equal(lv.cpu().numpy(), want_levels), "levels"
    held(tag + "_fwd", out, bin_major(f64), bin_major(f32))
    grads = align_bwd(dev(bin_major(dout_np)), [f.shape for f in feats], "rows", rois, levels, P, sampling)
    for l, g in enumerate(grads):
        held("%s_bwd_l%d" % (tag, l), torch.as_tensor(np.ascontiguousarray(g)), g64[l], g32[l])
    return out, f64, g64


@pytest.mark.parametrize("P,sampling", SC.SZ_OUT_CASES + SC.SZ_GRID_CASES)
def test_roi_align_sizes(P, sampling):
    """out_size 1 and 32 (lane 63 holds the last Wx), 2 and 31; the fixed grids 8 (the dense walk's last), 9 and 64 (the cap)"""
    _, f64, g64 = run_sizes("sizes_p%d_s%d" % (P, sampling), SC.SZ_ROIS, SC.SZ_LEVELS, P, sampling, SC.size_dout(P), SC.SZ_LEVELS)
    assert np.abs(f64).max() > 0.05 and all(np.abs(g).max() > 0.05 for g in g64)


def test_roi_align_levels_outside_are_clamped():
    clamped = np.clip(SC.SZ_BAD_LEVELS, 0, len(AL_SIZES) - 1)
    assert (clamped != SC.SZ_BAD_LEVELS).any()
    run_sizes("sizes_bad_levels", SC.SZ_ROIS, SC.SZ_BAD_LEVELS, 7, 2, SC.size_dout(7), clamped)


def test_roi_align_unusable_image_index():
    """rois[:, 0] of -1, 2 (= images) and NaN: a zero row, level -1 and no gradient, whatever dout holds there"""
    rois = SC.bad_image_rois()
    gone = sorted(SC.SZ_BAD_IMAGES)
    d = SC.size_dout(7)
    d[gone] *= F32(1e3)
    want = SC.SZ_LEVELS.copy()
    want[gone] = -1
    out, _, _ = run_sizes("sizes_bad_images", rois, SC.SZ_LEVELS, 7, 2, d, want)
    assert not out[gone].any()


# ------------------------------------------------------------------------------------------------------------------- the mask loss
def run_mask_loss(tag, c, z, n_pos_dev, n_pos_ref, M):
    """mtp_mask_loss on the fixed slots of a case against mask_ref with the counts n_pos_ref; n_pos_dev: what the device is handed"""
    B, S = c["sample_gt"].shape
    n, K = B * S, z.shape[1]
    use, r64, r32 = SC.slot_refs(c, z, n_pos_ref, M)
    assert SC.avg_margin(c, n_pos_ref, M) > MC.MARGIN, "the case keeps its target averages away from the threshold"
    got = dict(loss=ARENA.empty(1), targets=ARENA.empty(n, M, M, dtype=torch.uint8), slot_loss=ARENA.empty(n), target_avg=ARENA.empty(n, M, M))
    dl = ARENA.empty(n, K, M, M)
    ops.mask_loss(dev(z), dev(c["boxes"]), dev(c["labels"]), dev(c["sample_gt"]), dev(np.asarray(n_pos_dev, np.int64)), dev(c["bitmaps"]),
                  loss_weight=MC.LOSS_WEIGHT, dlogits=dl, out=got)
    for k in ("loss", "slot_loss", "target_avg"):
        ARENA.check_written(got[k])
    ARENA.check_written(dl)
    assert np.array_equal(got["targets"].cpu().numpy(), r64["targets"]), "targets, bit for bit"
    held(tag + "_avg", got["target_avg"], r64["avg"], r32["avg"])
    held(tag + "_slot", got["slot_loss"], r64["slot"], r32["slot"])
    held(tag + "_loss", got["loss"], r64["loss"], r32["loss"])
    held(tag + "_dlogits", dl, r64["d"], r32["d"])
    pad = torch.as_tensor(~use)
    assert not dl[pad].any() and not got["slot_loss"][pad].any() and not got["targets"][pad].any(), "padding slots are zero"
    other = np.ones((n, K), bool)
    other[np.arange(n), c["labels"]] = False
    assert not dl[torch.as_tensor(other)].any(), "the other class channels are zero"
    return got, r64


@pytest.mark.parametrize("M", SC.ML_SIZES)
def test_mask_loss_mask_sizes(M):
    """M M = 1 and 4 (one wave does everything, the others add zeros), 256 (every thread once), 289 (a second trip of 33 threads)"""
    c = SC.size_case(M)
    z = SC.loss_logits(len(c["boxes"]), MC.K, M, 40 + M)
    _, r64 = run_mask_loss("mask_loss_m%d" % M, c, z, c["n_pos"], c["n_pos"], M)
    assert float(r64["loss"][0]) > 0.1


def test_mask_loss_slots_beyond_one_trip_of_the_sum():
    c = SC.slots_case()
    got, r64 = run_mask_loss("mask_loss_99_slots", c, c["logits"], c["n_pos"], c["n_pos"], MC.M)
    assert r64["slot"][64:].max() > 0 and float(got["slot_loss"][64:].max()) > 0


def test_mask_loss_n_pos_is_clamped_on_the_device():
    c = SC.clamp_case()
    z = SC.loss_logits(len(c["boxes"]), MC.K, MC.M, 17)
    run_mask_loss("mask_loss_clamped", c, z, SC.CLAMP_GIVEN, SC.CLAMP_MEANT, MC.M)


# ------------------------------------------------------------------------------------------------------------------- the paste
@pytest.mark.parametrize("threshold", [MC.THR, 0.0, -1.0])
def test_mask_paste_zero_over_zero(threshold):
    """a zero-width box on the centre of pixel column 10: 0 / 0 there, a NaN value as the reference has it and an empty mask at any threshold"""
    logits, labels, boxes, h, w = SC.paste_case()
    N = len(boxes)
    out, vals = ARENA.empty(N, h, w, dtype=torch.uint8), ARENA.empty(N, h, w)
    masks = ops.mask_paste(dev(logits), dev(labels), dev(boxes), h, w, threshold, out=out, values=vals)
    v64, m64 = MR.paste(logits, labels, boxes, h, w, threshold)
    v32, _ = MR.paste(logits, labels, boxes, h, w, threshold, ft=F32)
    nan = np.isnan(v64)
    got = vals.cpu().numpy()
    assert nan.sum() == h and np.array_equal(np.isnan(got), nan), "NaN exactly where the reference has it"
    ARENA.check_written(vals)      # the poison is a NaN of a payload of its own: none of it is left
    fill = lambda a: np.where(nan, 0.0, a)      # noqa: E731
    held("mask_paste_nan_%s" % ("u8" if threshold < 0 else "thr%g" % threshold), torch.as_tensor(fill(got)), fill(v64), fill(v32).astype(F32))
    m = masks.cpu().numpy()
    assert not m[nan].any(), "empty where the value is a NaN"
    if threshold >= 0:
        off = ~nan & ((np.abs(v64 - threshold) > MC.MARGIN) | (v64 == 0))      # the padding's exact 0 is on the threshold 0.0 and passes it by right
        assert masks.dtype == torch.bool and np.array_equal(m[off], m64[off]) and off.sum() > 0.99 * off.size
    else:
        assert masks.dtype == torch.uint8 and int(np.abs(m.astype(np.int64) - m64.astype(np.int64)).max()) <= 1, "uint8 within one count"


# ------------------------------------------------------------------------------------------------------------------- the box half
@pytest.mark.parametrize("S", SC.RL_S)
def test_rpn_loss_chunks(S):
    """S = 256: one exactly full chunk of 256 slots per image; 257: one slot in a second chunk; 520: three chunks, a positive in each"""
    c = SC.rpn_loss_case(S)
    r64, r32 = SC.rpn_loss_refs(c)
    sgt, off = -np.ones((HC.BATCH, S), np.int64), 0
    for b, p in enumerate(c["n_pos"]):
        sgt[b, :p] = np.arange(p) + off
        off += p
    t_cls, t_reg = [ops.rpn_map_nchw(dev(m)) for m in c["cls"]], [ops.rpn_map_nchw(dev(m)) for m in c["reg"]]
    args = (dev(HC.priors(F32)), dev(np.concatenate(c["gts"])), dev(c["samples"]), dev(sgt), dev(c["n_pos"]), dev(c["n_neg"]))
    runs = []
    for _ in range(2):
        dcls, dreg = [ARENA.zeros(*m.shape) for m in c["cls"]], [ARENA.zeros(*m.shape) for m in c["reg"]]
        lc, lb = ops.hrpn_loss(t_cls, t_reg, HC.SIZES, HC.A, *args, HC.RPN_MEANS, HC.RPN_STDS, dcls=[ops.rpn_map_nchw(d) for d in dcls],
                               dreg=[ops.rpn_map_nchw(d) for d in dreg], loss_cls=ARENA.empty(len(HC.SIZES)), loss_bbox=ARENA.empty(len(HC.SIZES)))
        ARENA.check_written(lc)
        ARENA.check_written(lb)
        runs.append([lc, lb] + dcls + dreg)
    assert all(same_bits(a, b) for a, b in zip(*runs)), "two runs: the same bits"
    lc, lb, dcls, dreg = runs[0][0], runs[0][1], runs[0][2:2 + len(HC.SIZES)], runs[0][2 + len(HC.SIZES):]
    held("rpn_loss_s%d_cls" % S, lc, r64[0], r32[0])
    held("rpn_loss_s%d_bbox" % S, lb, r64[1], r32[1])
    for l in range(len(HC.SIZES)):
        held("rpn_loss_s%d_dcls_%d" % (S, l), dcls[l], r64[2][l], r32[2][l])
        held("rpn_loss_s%d_dreg_%d" % (S, l), dreg[l], r64[3][l], r32[3][l])
        assert not dcls[l].cpu().numpy()[r64[2][l] == 0].any() and not dreg[l].cpu().numpy()[r64[3][l] == 0].any(), "zero off the sampled anchors"
        assert np.array_equal(np.sign(dreg[l].cpu().numpy()), np.sign(r64[3][l])), "L1: the sign is the gradient"


def roi_loss_run(cls, reg, K, s, reg_target):
    """-> losses (3), dcls (R, K + 1), dreg (R, 4 K): column slices of one wide poisoned buffer, as the head lays them out"""
    n = len(cls)
    c0 = -(-(K + 1) // 4) * 4      # the deltas start on a 16-byte boundary
    buf, dbuf = ARENA.wide(n, c0 + 4 * K + 4), ARENA.wide(n, c0 + 4 * K + 4)
    t_cls, t_reg = ARENA.cols(buf, 0, K + 1), ARENA.cols(buf, c0, c0 + 4 * K)
    t_cls.copy_(torch.as_tensor(cls))
    t_reg.copy_(torch.as_tensor(reg))
    ARENA.frozen(buf)
    dcls, dreg = ARENA.cols(dbuf, 0, K + 1), ARENA.cols(dbuf, c0, c0 + 4 * K)
    losses = ops.hroi_loss(t_cls, t_reg, K, dev(np.ascontiguousarray(s["rois"][:, 1:])), dev(s["gts"]), dev(s["gt_labels"]), dev(s["sample_gt"]), dev(s["n_pos"]),
                           dev(s["n_neg"]), HC.ROI_MEANS, HC.ROI_STDS, reg_target, dcls=dcls, dreg=dreg, losses=ARENA.empty(3))
    ARENA.check_written(losses)
    return losses, dcls, dreg


@pytest.mark.parametrize("reg_target", ["reference", "encoded"])
@pytest.mark.parametrize("B,S,K", list(SC.RS_CASES))
def test_roi_loss_partial_rows(B, S, K, reg_target):
    """257, 260 and 1024 rows: 65 and 256 partial rows for the 64 lanes of the sum, a positive among the rows of the second trip"""
    cls, reg, s = SC.roi_loss_case(B, S, K)
    r64, r32 = SC.roi_loss_refs(cls, reg, K, s, reg_target)
    got = roi_loss_run(cls, reg, K, s, reg_target)
    again = roi_loss_run(cls, reg, K, s, reg_target)
    assert all(same_bits(a, b) for a, b in zip(again, got)), "two runs: the same bits"
    losses, dcls, dreg = got
    tag = "roi_loss_%dx%d_k%d_%s" % (B, S, K, reg_target)
    for i, k in enumerate(("loss_cls", "loss_bbox", "acc")):
        held("%s_%s" % (tag, k), losses[i].reshape(1), np.asarray(r64[k]).reshape(1), np.asarray(r32[k]).reshape(1))
    held(tag + "_dcls", dcls, r64["dcls"], r32["dcls"])
    held(tag + "_dreg", dreg, r64["dreg"], r32["dreg"])
    d = dreg.cpu().numpy()
    assert not np.isnan(d).any() and not d[r64["dreg"] == 0].any() and np.array_equal(np.sign(d), np.sign(r64["dreg"]))


def test_rpn_proposals_over_workgroups():
    """526 slots: three workgroups, the image boundary and every level's keep_first inside one"""
    cls, reg, _ = HC.planted()
    keep, counts = SC.proposal_keep(cls)
    B, T = len(keep), sum(counts)
    refs = SC.proposal_refs(cls, reg, keep)
    t_keep = dev(np.stack([np.concatenate(k) for k in keep]).astype(np.int64))
    t_cls, t_reg = [ops.rpn_map_nchw(dev(m)) for m in cls], [ops.rpn_map_nchw(dev(m)) for m in reg]
    priors, shapes = dev(HC.priors(F32)), dev(np.array([HC.IMG] * B, F32))
    for min_size in SC.PROP_MIN_SIZES:
        assert SC.proposal_size_condition(cls, reg, keep, min_size)
        out = (ARENA.empty(B, T), ARENA.empty(B, T, 4), ARENA.empty(B, T, dtype=torch.int64), ARENA.empty(B, T, dtype=torch.uint8))
        scores, boxes, ids, valid = ops.hrpn_proposals(t_cls, t_reg, HC.SIZES, HC.A, priors, t_keep, counts, HC.RPN_MEANS, HC.RPN_STDS, shapes, min_size, out=out)
        for t in (scores, boxes, ids):
            ARENA.check_written(t)
        for b, ((s64, b64, i64), (s32, b32, _)) in enumerate(refs):
            held("prop_526_scores_%d_min%g" % (b, min_size), scores[b], s64, s32)
            held("prop_526_boxes_%d_min%g" % (b, min_size), boxes[b], b64, b32)
            assert ids[b].tolist() == i64.tolist(), "level ids"
            want = ((b64[:, 2] - b64[:, 0]) > min_size) & ((b64[:, 3] - b64[:, 1]) > min_size)
            assert valid[b].bool().tolist() == want.tolist(), "the size flag"
            assert set(valid[b].unique().tolist()) <= {0, 1}
