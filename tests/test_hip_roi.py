"""GPU: the oriented RoI head (csrc/roi_head.hip, mtp_amd.ops_roi, roi_extractors, roi_heads, task_modules.DeltaXYWHTRBBoxCoder), every op buffer out of
a guard.Arena (poisoned outputs, guards on both sides, frozen inputs, the wrappers' own workspaces included).  The references are fixture f23 (the
reference's own RoI head, tests/golden/make_oriented_roi.py) for the sampling flow, the backward, loss_and_grads and predict, and tests/roi_ref.py in
float64 for the operators alone; the inputs are those of tests/roi_cases.py, whose conditions tests/test_roi_host.py asserts.
  1. RoIAlignRotated forward in NCHW strides and in row strides (same bits), kernel-computed and overridden levels, padded slots zero;
  2. its backward, alone and against f23's map gradients: zero off the touched pixels, accumulate adds, two calls bit-identical, the module's .backward() agrees;
  3. the coder: encode and decode against roi_ref, both clamps and the edge swap;
  4. gen_sampling_results with f23's recorded choice injected (gts prepended, lists equal to the reference's) and without (counts, membership, no
     duplicates, no host synchronisation); proposal lists padded behind a device-side count;
  5. loss_and_grads against f23: losses, acc, the gradients on maps and parameters, the image without gts, no host synchronisation;
  6. predict against f23: kept candidates and labels exact, boxes and scores close; a score_thr that removes candidates and a max_per_img that cuts;
  7. the layers against the same layers in numpy on the CPU, fp32 and with bf16-rounded operands;
  8. the head chained after MTP_RD_OrientedRPNHead: proposals -> losses, gradients of the maps, detections.
Every bound is 4 x the error of the float32 CPU restatement against float64 (floor 1e-6), computed here; both numbers are recorded."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import guard
import roi_cases as RC
import roi_ref as R
from conftest import record_parity
from mtp_amd import MODELS, ops
from mtp_amd.ops_roi import RoIAlignRotated
from mtp_amd.task_modules import DeltaXYWHTRBBoxCoder

pytestmark = pytest.mark.gpu
CASES = list(RC.SHAPES)
ARENA = None
GEOM = dict(out_size=RC.P, sample_num=RC.S, clockwise=RC.CLOCKWISE, finest_scale=RC.FINEST)
SCALES = [1.0 / s for s in RC.STRIDES]


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
def yard():
    """the float32 CPU run of every case: its distance from the float64 run is the yardstick"""
    return {n: RC.run(RC.case(n), np.float32) for n in CASES}


@pytest.fixture(scope="module")
def f23(golden):
    return golden("f23_oriented_roi.npz")


def recorded(f23, name):
    """the reference sampler's choice: per image (pos_inds, neg_inds) into [gts; proposals]"""
    return [(f23["%s.image%d.pos_inds" % (name, b)], f23["%s.image%d.neg_inds" % (name, b)]) for b in range(RC.BATCH)]


def slots(f23, name):
    """the fixed-size lists' rows in use (B NUM) bool: image b holds its n_pos + n_neg recorded samples first"""
    v = np.zeros(RC.BATCH * RC.NUM, bool)
    for b, (pos, neg) in enumerate(recorded(f23, name)):
        v[b * RC.NUM:b * RC.NUM + len(pos) + len(neg)] = True
    return v


def padded(f23, name, key, dtype=np.float64):
    """a per-sample record of f23 (the reference has no padding) in the fixed-size layout, zeros on the padding"""
    a, v = f23[name + "." + key], slots(f23, name)
    out = np.zeros((len(v),) + a.shape[1:], dtype)
    out[v] = a
    return out


def dev(a):
    """an op INPUT on the device, frozen"""
    return ARENA.frozen(ARENA.like(torch.as_tensor(np.ascontiguousarray(a))))


def err_of(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a.astype(np.float64) - ref).max()) if ref.size else 0.0


def held(tag, out, ref64, ref32):
    """4 x the float32 CPU error of the restatement against float64, floor 1e-6"""
    ref64 = np.asarray(ref64, np.float64)
    err, e32 = err_of(out, ref64), err_of(ref32, ref64)
    record_parity("roi", tag, err)
    record_parity("roi", "roi_ref_f32_cpu_" + tag, e32)
    print("%s: err %.3e, float32 restatement %.3e" % (tag, err, e32))
    assert tuple(out.shape) == ref64.shape and err < max(4 * e32, 1e-6), (tag, err, e32)


def bin_major(x):
    """(R, C, P, P) -> the kernels' (R, P P, C)"""
    return np.ascontiguousarray(np.transpose(x.reshape(x.shape[0], x.shape[1], -1), (0, 2, 1)))


def rows_of(maps, ld):
    """NCHW maps -> per level (N H W, ld) rows whose first C columns are the channels"""
    out = []
    for m in maps:
        N, Cc, H, W = m.shape
        r = np.zeros((N * H * W, ld), np.float32)
        r[:, :Cc] = np.transpose(m, (0, 2, 3, 1)).reshape(-1, Cc)
        out.append(r)
    return out


def make_head(precision="fp32", num_classes=RC.K, weights=None, test_cfg=None):
    cfg = dict(
        type="MTP_RD_StandardRoIHead",
        bbox_roi_extractor=dict(type="RotatedSingleRoIExtractor", roi_layer=dict(type="RoIAlignRotated", out_size=RC.P, sample_num=RC.S, clockwise=RC.CLOCKWISE),
                                out_channels=RC.C, featmap_strides=list(RC.STRIDES)),
        bbox_head=dict(type="MTP_RD_Shared2FCBBoxHead", predict_box_type="rbox", in_channels=RC.C, fc_out_channels=RC.FC_OUT, roi_feat_size=RC.P,
                       reg_predictor_cfg=dict(type="mmdet.Linear"), cls_predictor_cfg=dict(type="mmdet.Linear"),
                       bbox_coder=dict(type="mmrotate.DeltaXYWHTRBBoxCoder", angle_version="le90", norm_factor=None, edge_swap=True, proj_xy=True,
                                       target_means=RC.MEANS, target_stds=RC.STDS),
                       reg_class_agnostic=True, loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                       loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=RC.BETA, loss_weight=1.0), precision=precision),
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="mmrotate.RBboxOverlaps2D"), **RC.ASSIGNER),
                       sampler=dict(type="RandomSampler", num=RC.NUM, pos_fraction=RC.POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=True),
                       pos_weight=-1, debug=False),
        test_cfg=dict(test_cfg or RC.RCNN))
    if num_classes is not None:
        cfg["bbox_head"]["num_classes"] = num_classes
    head = MODELS.build(cfg).cuda()
    if weights is not None:
        sd = {"bbox_head." + k: torch.as_tensor(v) for k, v in weights.items() if num_classes is not None or k.startswith("shared_fcs.")}
        head.load_state_dict(sd)
    return head


def inputs(name):
    c = RC.case(name)
    feats = [dev(f) for f in c["feats"]]
    gts = [NS(rboxes=dev(g.reshape(-1, 5)), rlabels=dev(l)) for g, l in zip(c["gts"], c["labels"])]
    props = [NS(bboxes=dev(p)) for p in c["props"]]
    return c, feats, gts, props


def choice(name):
    """roi_cases' restatement of the reference sampler's choice (tests/test_roi_host.py holds it equal to f23's)"""
    return [(s["pos"], s["neg"]) for s in RC.sampling(RC.case(name))[0]]


# ------------------------------------------------------------------------------------------------------------------- 1. RoIAlignRotated forward
@pytest.mark.parametrize("channels", [RC.C, RC.C_WIDE])
def test_roi_align_forward(channels):
    maps, rois = RC.align_case()
    maps = maps[channels]
    sizes, N, Rn = [m.shape[2:] for m in maps], RC.BATCH, len(rois)
    t_rois = dev(rois)
    nchw = [ops.rpn_map_nchw(dev(m)) for m in maps]
    ld = channels + 4
    rows = [ops.rpn_map_rows(dev(r), H, W) for r, (H, W) in zip(rows_of(maps, ld), sizes)]
    levels = R.map_levels(rois, len(maps), RC.FINEST)
    other = (levels + 1) % len(maps)
    for tag, lv in (("computed", None), ("override", other)):
        t_lv = None if lv is None else dev(lv.astype(np.int32))
        ref = bin_major(R.roi_align(maps, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, levels=lv))
        ref32 = bin_major(R.roi_align(maps, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, levels=lv, dtype=np.float32))
        used = ARENA.empty(Rn, dtype=torch.int32)
        a = ops.roi_align_rotated_fwd(nchw, sizes, SCALES, channels, N, t_rois, roi_levels=t_lv, out=ARENA.empty(Rn, RC.P * RC.P, channels), levels_out=used, **GEOM)
        b = ops.roi_align_rotated_fwd(rows, sizes, SCALES, channels, N, t_rois, roi_levels=t_lv, **GEOM)
        held("align_%s_%d" % (tag, channels), a, ref, ref32)
        assert torch.equal(a, b) and used.tolist() == (levels if lv is None else lv).tolist()
    assert not ref[7].any() and np.abs(ref).max() > 0.5      # the RoI wholly outside is all zeros (the last run: its overridden level too)
    # padded slots: two groups of Rn / 2 slots with Rn / 2 and 5 in use; the rest writes zeros, whatever its RoI says
    valid = np.zeros(Rn, bool)
    valid[:Rn // 2] = True
    valid[Rn // 2:Rn // 2 + 5] = True
    junk = rois.copy()
    junk[~valid, 1:] = np.nan
    out = ops.roi_align_rotated_fwd(nchw, sizes, SCALES, channels, N, dev(junk), valid=dev(np.array([Rn // 2, 5])), **GEOM)
    ref = bin_major(R.roi_align(maps, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, valid=valid))
    ref32 = bin_major(R.roi_align(maps, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, valid=valid, dtype=np.float32))
    held("align_padded_%d" % channels, out, ref, ref32)
    assert not out[torch.as_tensor(~valid).cuda()].any()


def test_roi_align_module_and_empty():
    maps, rois = RC.align_case()
    with pytest.raises(NotImplementedError):
        RoIAlignRotated(7, 0.25, sample_num=0)
    with pytest.raises(NotImplementedError):
        RoIAlignRotated(7, 0.25, sample_num=2, aligned=False)
    layer = RoIAlignRotated(output_size=RC.P, spatial_scale=0.25, sampling_ratio=RC.S, clockwise=RC.CLOCKWISE)
    x = torch.as_tensor(maps[RC.C][0])
    assert tuple(layer(x, torch.zeros(0, 6)).shape) == (0, RC.C, RC.P, RC.P)      # R = 0: on any device, the library untouched
    ex = MODELS.build(dict(type="mmrotate.RotatedSingleRoIExtractor", roi_layer=dict(type="RoIAlignRotated", out_size=RC.P, sample_num=RC.S, clockwise=True),
                           out_channels=RC.C, featmap_strides=list(RC.STRIDES)))
    assert tuple(ex([torch.as_tensor(m) for m in maps[RC.C]], torch.zeros(0, 6)).shape) == (0, RC.C, RC.P, RC.P) and ex.num_inputs == 4
    with pytest.raises(NotImplementedError):
        ex([torch.as_tensor(m) for m in maps[RC.C]], torch.zeros(0, 6), roi_scale_factor=1.2)
    feats = [dev(m) for m in maps[RC.C]]
    out = ex(feats, dev(rois))
    ref = R.roi_align(maps[RC.C], rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST)
    held("extractor", out, ref, R.roi_align(maps[RC.C], rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, dtype=np.float32))
    assert ex.map_roi_levels(dev(rois), 4).tolist() == R.map_levels(rois, 4, RC.FINEST).tolist()


# ------------------------------------------------------------------------------------------------------------------- 2. RoIAlignRotated backward
@pytest.mark.parametrize("channels", [RC.C, RC.C_WIDE])
def test_roi_align_backward(channels):
    maps, rois = RC.align_case()
    maps = maps[channels]
    sizes, N, Rn = [m.shape[2:] for m in maps], RC.BATCH, len(rois)
    rng = np.random.default_rng(5)
    dout = rng.normal(0, 1, (Rn, channels, RC.P, RC.P)).astype(np.float32)
    shapes = [m.shape for m in maps]
    ref = R.roi_align_bwd(dout, shapes, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST)
    ref32 = R.roi_align_bwd(dout, shapes, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, dtype=np.float32)
    t_rois, t_dout = dev(rois), dev(bin_major(dout))

    def run(bufs, accumulate=False):
        ops.roi_align_rotated_bwd(t_dout, [ops.rpn_map_nchw(b) for b in bufs], sizes, SCALES, channels, N, t_rois, accumulate=accumulate, **GEOM)
        return bufs
    g = run([ARENA.zeros(*s) for s in shapes])
    for l in range(len(maps)):
        held("align_bwd_%d_%d" % (channels, l), g[l], ref[l], ref32[l])
        assert not g[l].cpu().numpy()[ref[l] == 0].any() and (ref[l] != 0).any()      # exactly zero off the touched pixels
    again = run([ARENA.zeros(*s) for s in shapes])
    assert all(torch.equal(a, b) for a, b in zip(again, g))      # two calls: the same bits
    base = [rng.normal(0, 1, s).astype(np.float32) for s in shapes]
    acc = run([ARENA.like(torch.as_tensor(b)) for b in base], accumulate=True)
    for a, b, gl, r in zip(acc, base, g, ref):
        want = torch.as_tensor(b).cuda() + gl
        assert torch.equal(a, want) and np.array_equal(a.cpu().numpy()[r == 0], b[r == 0])
    # row strides: the same bits
    ld = channels + 4
    rows = [ARENA.zeros(N * H * W, ld) for H, W in sizes]
    ops.roi_align_rotated_bwd(t_dout, [ops.rpn_map_rows(r, H, W) for r, (H, W) in zip(rows, sizes)], sizes, SCALES, channels, N, t_rois, **GEOM)
    for r, gl, (H, W) in zip(rows, g, sizes):
        assert torch.equal(r[:, :channels].reshape(N, H, W, channels).permute(0, 3, 1, 2), gl) and not r[:, channels:].any()


@pytest.mark.parametrize("name", CASES)
def test_roi_align_backward_vs_f23(f23, name, yard):
    """the reference's recorded gradient of the RoI features through the backward launches -> its recorded gradients of the maps"""
    c = RC.case(name)
    v = slots(f23, name)
    rois = padded(f23, name, "rois", np.float32)
    rois[:, 0] = np.repeat(np.arange(RC.BATCH), RC.NUM)
    dout = padded(f23, name, "d_bbox_feats", np.float32)
    sizes, shapes = [f.shape[2:] for f in c["feats"]], [f.shape for f in c["feats"]]
    bufs = [ARENA.zeros(*s) for s in shapes]
    counts = dev(np.array([v[b * RC.NUM:(b + 1) * RC.NUM].sum() for b in range(RC.BATCH)], np.int64))
    ops.roi_align_rotated_bwd(dev(bin_major(dout)), [ops.rpn_map_nchw(b) for b in bufs], sizes, SCALES, RC.C, RC.BATCH, dev(rois), valid=counts, **GEOM)
    ref32 = R.roi_align_bwd(dout, shapes, rois, RC.STRIDES, RC.P, RC.S, RC.CLOCKWISE, RC.FINEST, valid=v, dtype=np.float32)
    for l, b in enumerate(bufs):
        want = f23["%s.level%d.dfeat" % (name, l)]
        held("%s_align_bwd_f23_%d" % (name, l), b, want, ref32[l])
        assert not b.cpu().numpy()[want == 0].any()


def test_roi_align_module_backward():
    """the nn.Module on one level: the RoIs of the case that map to level 0, through autograd"""
    maps, rois = RC.align_case()
    m = maps[RC.C][0]
    rois = rois[R.map_levels(rois, 4, RC.FINEST) == 0]
    assert len(rois) >= 4
    rng = np.random.default_rng(6)
    dout = rng.normal(0, 1, (len(rois), RC.C, RC.P, RC.P)).astype(np.float32)
    layer = RoIAlignRotated(RC.P, 1.0 / RC.STRIDES[0], sample_num=RC.S, clockwise=RC.CLOCKWISE)
    x = torch.as_tensor(m).cuda().requires_grad_()
    out = layer(x, dev(rois))
    out.backward(dev(dout))
    lv = np.zeros(len(rois), np.int64)
    args = (rois, RC.STRIDES[:1], RC.P, RC.S, RC.CLOCKWISE, RC.FINEST)
    held("module_fwd", out.detach(), R.roi_align([m], *args, levels=lv), R.roi_align([m], *args, levels=lv, dtype=np.float32))
    held("module_bwd", x.grad, R.roi_align_bwd(dout, [m.shape], *args, levels=lv)[0], R.roi_align_bwd(dout, [m.shape], *args, levels=lv, dtype=np.float32)[0])


# ------------------------------------------------------------------------------------------------------------------- 3. the coder
def coder_inputs(n, seed):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(20, 100, (n, 2)), rng.uniform(8, 60, (n, 2)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1).astype(np.float32)
    g = np.concatenate([p[:, :2] + rng.uniform(-6, 6, (n, 2)), rng.uniform(8, 60, (n, 2)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1).astype(np.float32)
    return p, g


@pytest.mark.parametrize("n", [1, 65, 600])
def test_coder_encode(n):
    p, g = coder_inputs(3 * n, 40 + n)
    gap, wrap = R.angle_margins(p, g)      # the choice between d1 and d2 is made in float64: inputs clear of it (chosen before anything runs)
    d = g[:, 4].astype(np.float64) - p[:, 4]
    fine = (gap > RC.ANGLE_GAP) & (np.abs(np.abs(R.norm_angle(d)) - np.pi / 2) > RC.ANGLE_GAP) & (np.abs(np.abs(R.norm_angle(d + np.pi / 2)) - np.pi / 2) > RC.ANGLE_GAP)
    p, g = p[fine][:n], g[fine][:n]
    assert len(p) == n
    for tag, means, stds in (("", RC.MEANS, RC.STDS), ("means_", (0.1, -0.2, 0.3, 0.0, 0.05), (0.5, 0.5, 0.25, 0.25, 0.3))):
        out = DeltaXYWHTRBBoxCoder(target_means=means, target_stds=stds).encode(dev(p), dev(g))
        held("encode_%s%d" % (tag, n), out, R.encode(p, g, means, stds), R.encode(p, g, means, stds, np.float32))
    coder = DeltaXYWHTRBBoxCoder(target_means=RC.MEANS, target_stds=RC.STDS)
    assert tuple(coder.encode(torch.zeros(0, 5, device="cuda"), torch.zeros(0, 5, device="cuda")).shape) == (0, 5) and coder.encode_size == 5


@pytest.mark.parametrize("n", [1, 65, 600])
def test_coder_decode(n):
    rng = np.random.default_rng(50 + n)
    p = coder_inputs(3 * n + 24, 60 + n)[0]
    d = rng.normal(0, 1.0, (len(p), 5)) * np.array([1, 1, 2, 2, 4])
    if n > 20:      # both clamps: sizes beyond exp(+-|log(16 / 1000)|) / std
        d[:6, 2], d[:6, 3] = [45, -45, 25, 21, -21, 0], [0, 45, -45, -25, 21, -21]
    d = d.astype(np.float32)
    ref, gw, gh, ga = R.decode(p, d, RC.MEANS, RC.STDS, swapped=True)
    fine = (np.abs(gw - gh) > RC.SHAPE_GAP * np.maximum(gw, gh)) & (np.abs(np.abs(ga) - np.pi / 2) > RC.ANGLE_GAP) & (np.abs(np.abs(ref[:, 4]) - np.pi / 2) > RC.ANGLE_GAP)
    fine[:6] &= n > 20
    keep = np.concatenate([np.nonzero(fine[:6])[0], 6 + np.nonzero(fine[6:])[0][:n]])
    p, d, ref = p[keep], d[keep], ref[keep]
    assert len(p) >= n and (n <= 20 or fine[:6].sum() >= 4)      # the clamped rows are among what is compared
    sw = gw[keep] > gh[keep]
    assert n < 20 or (sw.any() and (~sw).any())      # both sides of the edge swap
    out = DeltaXYWHTRBBoxCoder(target_means=RC.MEANS, target_stds=RC.STDS).decode(dev(p), dev(d), max_shape=(128, 128))
    held("decode_%d" % n, out, ref, R.decode(p, d, RC.MEANS, RC.STDS, np.float32))
    assert (out[:, 2] >= out[:, 3]).all() and (out[:, 4] >= -np.pi / 2).all() and (out[:, 4] < np.pi / 2).all()


# ------------------------------------------------------------------------------------------------------------------- 4. sampling
@pytest.mark.parametrize("name", CASES)
def test_sampling_with_the_choice_injected(f23, name):
    c, feats, gts, props = inputs(name)
    head = make_head(weights=c["W"])
    s = head.gen_sampling_results(props, gts, sample_inds=recorded(f23, name))
    v = torch.as_tensor(slots(f23, name)).cuda()
    off = 0
    for b, (pos, neg) in enumerate(recorded(f23, name)):      # the lists of the reference: its positives, then its negatives, into [gts; proposals]
        k, n = len(c["gts"][b]), len(pos) + len(neg)
        assert int(s["n_pos"][b]) == len(pos) and int(s["n_neg"][b]) == len(neg)
        assert s["inds"][b, :n].tolist() == list(pos) + list(neg)
        assert s["sample_gt"][b, :len(pos)].tolist() == (f23["%s.image%d.pos_gt" % (name, b)] + off).tolist() and (s["sample_gt"][b, len(pos):] == -1).all()
        assert all(f23["%s.image%d.pos_gt" % (name, b)][j] == i for j, i in enumerate(pos) if i < k)      # gt i, prepended, is assigned to itself
        off += k
    assert torch.equal(s["rois"][v], torch.as_tensor(f23[name + ".rois"].astype(np.float32)).cuda())      # the reference's rois, image index included
    assert s["rois"][:, 0].tolist() == np.repeat(np.arange(RC.BATCH), RC.NUM).tolist()
    assert torch.equal(s["gts"], torch.cat([g.rboxes for g in gts])) and torch.equal(s["gt_labels"], torch.cat([g.rlabels for g in gts]))
    want = RC.sample_lists(c)      # and roi_cases' own lists are those
    assert np.array_equal(want["valid"], slots(f23, name)) and s["n_pos"].tolist() == want["n_pos"].tolist()


def test_sampling_with_a_device_side_proposal_count():
    """proposal lists padded to a fixed length with .count on the device: the rows beyond it are never drawn, the injected choice gives the same lists"""
    name = "sq128"
    c, feats, gts, props = inputs(name)
    head = make_head(weights=c["W"])
    junk = np.tile(c["gts"][0][:1], (9, 1))      # copies of a gt: they would all be positives if they were looked at
    padded = [NS(bboxes=dev(np.concatenate([p, junk])), count=torch.tensor(RC.NUM_PROP, device="cuda")) for p in c["props"]]
    a, b = head.gen_sampling_results(props, gts, sample_inds=choice(name)), head.gen_sampling_results(padded, gts, sample_inds=choice(name))
    assert all(torch.equal(a[k], b[k]) for k in ("inds", "sample_gt", "n_pos", "n_neg")) and torch.equal(a["rois"], b["rois"])
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(4):
        r = head.gen_sampling_results(padded, gts, generator=g)
        for i in range(RC.BATCH):
            n = int(r["n_pos"][i] + r["n_neg"][i])
            assert (r["inds"][i, :n] < len(c["gts"][i]) + RC.NUM_PROP).all() and int(r["n_pos"][i]) == int(RC.NUM * RC.POS_FRACTION)


def test_sampling_without_a_host_synchronisation():
    name = "pad160"
    c, feats, gts, props = inputs(name)
    head = make_head(weights=c["W"])
    gens = [torch.Generator(device="cuda").manual_seed(s) for s in (3, 3, 4)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        runs = [head.gen_sampling_results(props, gts, generator=g) for g in gens]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    a, b, d = runs
    assert torch.equal(a["inds"], b["inds"]) and not torch.equal(a["inds"], d["inds"])      # the generator decides
    sm = RC.sampling(c)[0]
    for r in runs:
        for i, q in enumerate(sm):
            np_, nn = int(r["n_pos"][i]), int(r["n_neg"][i])
            cand_pos, cand_neg = set(np.nonzero(q["gt_inds"] > 0)[0].tolist()), set(np.nonzero(q["gt_inds"] == 0)[0].tolist())
            assert np_ == min(int(RC.NUM * RC.POS_FRACTION), len(cand_pos)) and nn == min(RC.NUM - np_, len(cand_neg))
            got = r["inds"][i, :np_ + nn].tolist()
            assert len(set(got)) == np_ + nn and set(got[:np_]) <= cand_pos and set(got[np_:]) <= cand_neg
            assert r["sample_gt"][i, :np_].tolist() == [int(q["gt_inds"][j]) - 1 + (0 if i == 0 else len(c["gts"][0])) for j in got[:np_]]
    assert int(runs[0]["n_pos"][1]) == 0      # the image without gts


# ------------------------------------------------------------------------------------------------------------------- 5. loss and gradients
@pytest.mark.parametrize("name", CASES)
def test_loss_and_grads(f23, name, yard):
    c, feats, gts, props = inputs(name)
    y32 = yard[name]
    head = make_head(weights=c["W"])
    pick = recorded(f23, name)
    v = slots(f23, name)
    bf, rois = head.train_bbox_forward(feats, head.gen_sampling_results(props, gts, sample_inds=pick))
    held(name + "_bbox_feats", bf, padded(f23, name, "bbox_feats"), y32["x"])
    assert not bf[torch.as_tensor(~v).cuda()].any()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # nothing between the proposals and the loss waits on the host
    try:
        losses, G, dfeats = head.loss_and_grads(feats, props, gts, generator=torch.Generator(device="cuda").manual_seed(1))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(t).all() for t in losses.values())
    losses, G, dfeats = head.loss_and_grads(feats, props, gts, sample_inds=pick)
    for k in ("loss_cls", "loss_bbox", "acc"):
        held("%s_%s" % (name, k), losses[k].reshape(1), np.asarray(f23["%s.%s" % (name, k)]).reshape(1), np.asarray(y32["loss"][k]).reshape(1))
    assert sorted(G) == sorted(n for n, _ in head.named_parameters()) and all(p.grad is None for p in head.parameters())
    for k in y32["G"]:
        held("%s_d_%s" % (name, k), G["bbox_head." + k], f23["%s.grad.%s" % (name, k)], y32["G"][k])
    for l in range(len(feats)):
        want = f23["%s.level%d.dfeat" % (name, l)]
        held("%s_dfeat_%d" % (name, l), dfeats[l], want, y32["dfeats"][l])
        assert not dfeats[l].cpu().numpy()[want == 0].any()
    if name == "pad160":      # the image without gts: negatives alone, labelled background, no box target
        tail = slice(len(pick[0][0]) + len(pick[0][1]), None)
        assert len(pick[1][0]) == 0 and len(pick[1][1]) == RC.NUM and (f23[name + ".labels"][tail] == RC.K).all() and not f23[name + ".bbox_weights"][tail].any()
    else:
        assert not v.all()      # padded slots
    # two calls: the same bits from the kernels of roi_head.hip and the data path (the bias gradients are the GEMMs' column-sum by-product, which
    # the GEMM launchers add with atomics in every head: they are held to the bound above, not to bit identity)
    again = head.loss_and_grads(feats, props, gts, sample_inds=pick)
    assert all(torch.equal(again[0][k], losses[k]) for k in losses) and all(torch.equal(a, b) for a, b in zip(again[2], dfeats))
    assert torch.equal(head.loss(feats, props, gts, sample_inds=pick)["loss_cls"], losses["loss_cls"])
    sr = head.gen_sampling_results(props, gts, sample_inds=pick)      # the reference's own call: bbox_loss on given scores and deltas
    out = head.bbox_loss(RC.K, sr, sr["rois"], dict(cls_score=dev(padded(f23, name, "cls_score", np.float32)), bbox_pred=dev(padded(f23, name, "bbox_pred", np.float32))))
    for k in ("loss_cls", "loss_bbox", "acc"):
        held("%s_bbox_loss_%s" % (name, k), out["loss_bbox"][k].reshape(1), np.asarray(f23["%s.%s" % (name, k)]).reshape(1), np.asarray(y32["loss"][k]).reshape(1))


def test_loss_with_predictors_passed_per_call():
    """the pretraining form: a head without num_classes, fc_cls and fc_reg owned by the caller"""
    name = "sq128"
    c, feats, gts, props = inputs(name)
    own, bare = make_head(weights=c["W"]), make_head(num_classes=None, weights=c["W"])
    assert sorted(bare.state_dict()) == ["bbox_head.shared_fcs.%d.%s" % (i, k) for i in (0, 1) for k in ("bias", "weight")]
    assert bare.bbox_head.cls_last_dim == bare.bbox_head.reg_last_dim == RC.FC_OUT
    fc_cls, fc_reg = torch.nn.Linear(RC.FC_OUT, RC.K + 1).cuda(), torch.nn.Linear(RC.FC_OUT, 5).cuda()
    with torch.no_grad():
        for m, k in ((fc_cls, "fc_cls"), (fc_reg, "fc_reg")):
            m.weight.copy_(torch.as_tensor(c["W"][k + ".weight"]))
            m.bias.copy_(torch.as_tensor(c["W"][k + ".bias"]))
    a = own.loss_and_grads(feats, props, gts, sample_inds=choice(name))
    b = bare.loss_and_grads(feats, props, gts, num_classes=RC.K, fc_cls=fc_cls, fc_reg=fc_reg, sample_inds=choice(name))
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[1]["bbox_head.fc_cls.weight"], b[1]["fc_cls.weight"]) and torch.equal(a[1]["bbox_head.shared_fcs.0.weight"], b[1]["bbox_head.shared_fcs.0.weight"])
    with pytest.raises(ValueError):
        bare.loss_and_grads(feats, props, gts, sample_inds=choice(name))
    x_cls, x_reg = bare.bbox_head(own.train_bbox_forward(feats, own.gen_sampling_results(props, gts, sample_inds=choice(name)))[0])
    assert tuple(x_cls.shape) == (RC.BATCH * RC.NUM, RC.FC_OUT) and x_cls is x_reg


# ------------------------------------------------------------------------------------------------------------------- 6. predict
@pytest.mark.parametrize("tag,cfg", [("det", RC.RCNN), ("det_thr", RC.RCNN_THR), ("det_cut", RC.RCNN_CUT)])
@pytest.mark.parametrize("name", CASES)
def test_predict(f23, name, tag, cfg, yard):
    c, feats, gts, props = inputs(name)
    y32 = yard[name]
    head = make_head(weights=c["W"], test_cfg=cfg)
    res = head.predict(feats, props)
    again = head.predict_bbox(feats, None, props, rcnn_test_cfg=cfg)
    for b, r in enumerate(res):
        q = "%s.%s.image%d." % (name, tag, b)
        keep = f23[q + "keep"]
        assert r.keep.tolist() == keep.tolist() and r.labels.tolist() == f23[q + "labels"].tolist()      # exact, in order
        t32, b32 = y32["dets"][tag][b][4:]
        held("%s_%s_boxes_%d" % (name, tag, b), r.bboxes, f23[q + "bboxes"], b32[keep // RC.K])
        held("%s_%s_scores_%d" % (name, tag, b), r.scores, f23[q + "scores"], t32.reshape(-1)[keep])
        assert (r.scores > cfg["score_thr"]).all() and 0 < len(r.scores) <= cfg["max_per_img"]
        assert torch.equal(again[b].keep, r.keep) and torch.equal(again[b].bboxes, r.bboxes) and torch.equal(again[b].scores, r.scores)
    if tag == "det":
        none = head.predict(feats, [NS(bboxes=torch.zeros(0, 5, device="cuda")) for _ in props])      # R = 0: empty results, the library untouched
        assert all(len(r.scores) == 0 and tuple(r.bboxes.shape) == (0, 5) for r in none)
        proposals, rois = head.test_bbox_generate_roi(props)
        out = head._bbox_forward(feats, rois)
        held(name + "_cls_score", out["cls_score"], f23[name + ".test.cls_score"], y32["tcls"])
        held(name + "_bbox_pred", out["bbox_pred"], f23[name + ".test.bbox_pred"], y32["treg"])
        held(name + "_test_feats", head.test_bbox_roi_feats(feats, rois), RC.reference(name)["xt"], y32["xt"])
    else:
        fewer = [len(f23["%s.det.image%d.keep" % (name, b)]) for b in range(RC.BATCH)]
        assert all(len(r.scores) < n for r, n in zip(res, fewer))      # the threshold removed candidates / max_per_img cut


# ------------------------------------------------------------------------------------------------------------------- 7. the layers
def bf16_round(a):
    return torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_layers_vs_cpu(precision):
    c = RC.case("sq128")
    rng = np.random.default_rng(8)
    Rn = 70
    x = rng.normal(0, 1, (Rn, RC.C, RC.P, RC.P)).astype(np.float32)
    dcls, dreg = rng.normal(0, 0.1, (Rn, RC.K + 1)).astype(np.float32), rng.normal(0, 0.1, (Rn, 5)).astype(np.float32)
    rnd = bf16_round if precision == "bf16" else None
    tc, tr, tctx = R.fc_forward(x.reshape(Rn, -1), c["W"])
    tG, tdx = R.fc_backward(dcls, dreg, tctx)
    yc, yr, yctx = R.fc_forward(x.reshape(Rn, -1), c["W"], np.float32, rnd)
    yG, ydx = R.fc_backward(dcls, dreg, yctx, np.float32)
    head = make_head(precision, weights=c["W"]).bbox_head
    cls, reg = head(dev(x))
    tag = "layers_%s_" % precision
    held(tag + "cls", cls, tc, yc)
    held(tag + "reg", reg, tr, yr)
    eng, out, ctx, K = head.forward_rows(head.rows_of(dev(x)))
    dout = torch.zeros_like(out)
    dout[:, :K + 1], dout[:, K + 1:K + 6] = torch.as_tensor(dcls).cuda(), torch.as_tensor(dreg).cuda()
    G = {n: torch.zeros_like(p) for n, p in head.named_parameters()}
    dx = eng.backward_rows(dout, ctx, G, head.predictors()[3])
    held(tag + "dx", dx, bin_major(tdx.reshape(x.shape)).reshape(Rn, -1), bin_major(ydx.reshape(x.shape)).reshape(Rn, -1))
    for k in G:
        held(tag + k, G[k], tG[k], yG[k])


def test_weight_image_cache_and_invalidate_weights():
    """the permuted image of shared_fcs.0.weight is kept per weight version: a write through torch is seen; a write that goes round the version
    counter (as the project's optimizer and broadcast kernels do) is seen after invalidate_weights()"""
    c = RC.case("sq128")
    head = make_head(weights=c["W"])
    bh = head.bbox_head
    x = dev(np.random.default_rng(1).normal(0, 1, (9, RC.C, RC.P, RC.P)).astype(np.float32))
    first = bh(x)[0].clone()
    assert torch.equal(bh(x)[0], first)
    with torch.no_grad():
        bh.shared_fcs[0].weight.mul_(0.5)      # through torch: the version counter moves
    second = bh(x)[0].clone()
    assert not torch.equal(second, first)
    bh.shared_fcs[0].weight.data.mul_(2.0)      # round the counter: the cached image is still the halved one
    assert torch.equal(bh(x)[0], second)
    head.invalidate_weights()
    assert torch.equal(bh(x)[0], first)      # halving and doubling are exact: the first weights again


# ------------------------------------------------------------------------------------------------------------------- chained after the RPN head
def test_chained_after_the_oriented_rpn_head():
    """five maps -> MTP_RD_OrientedRPNHead.predict -> proposals -> the RoI head on the first four maps: losses, gradients on those maps, detections"""
    import rpn_cases as PC
    rpn = MODELS.build(dict(
        type="MTP_RD_OrientedRPNHead", in_channels=RC.C, feat_channels=RC.C,
        anchor_generator=dict(type="mmdet.AnchorGenerator", scales=list(PC.SCALES), ratios=list(PC.RATIOS), strides=list(PC.STRIDES), use_box_type=True),
        bbox_coder=dict(type="MidpointOffsetCoder", angle_version="le90", target_means=list(PC.MEANS), target_stds=list(PC.STDS)),
        test_cfg=dict(PC.PROPOSAL))).cuda()
    c, feats, gts, _ = inputs("sq128")
    torch.manual_seed(3)
    five = feats + [torch.randn(RC.BATCH, RC.C, 2, 2, device="cuda")]
    proposals = rpn.predict(five, [dict(img_shape=(128, 128), pad_shape=(128, 128))] * RC.BATCH)
    assert all(0 < len(p.scores) <= PC.PROPOSAL["max_per_img"] and tuple(p.bboxes.shape[1:]) == (5,) for p in proposals)
    head = make_head(weights=c["W"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")      # between the proposals and the loss nothing waits on the host
    try:
        losses, G, dfeats = head.loss_and_grads(five, proposals, gts, generator=torch.Generator(device="cuda").manual_seed(2))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(v).all() for v in losses.values()) and float(losses["loss_cls"]) > 0 and 0 <= float(losses["acc"]) <= 100
    assert len(dfeats) == 4 and all(d.shape == f.shape and torch.isfinite(d).all() for d, f in zip(dfeats, feats)) and any(d.any() for d in dfeats)
    assert all(torch.isfinite(g).all() for g in G.values()) and G["bbox_head.shared_fcs.0.weight"].any()
    dets = head.predict(five, proposals)
    assert len(dets) == RC.BATCH and all(tuple(d.bboxes.shape) == (len(d.scores), 5) and d.labels.dtype == torch.int64 for d in dets)
    assert all((d.scores[:-1] >= d.scores[1:]).all() and (d.scores > RC.RCNN["score_thr"]).all() and (d.labels < RC.K).all() for d in dets)
