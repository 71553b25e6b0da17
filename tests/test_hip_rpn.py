"""GPU: the oriented RPN (csrc/rpn.hip, mtp_amd.task_modules, mtp_amd.dense_heads), every op buffer out of a guard.Arena (poisoned outputs, guards on both
sides, frozen inputs, the wrappers' own workspaces included).  The references are tests/rpn_ref.py in float64 and fixture f22 (the reference's own
head, tests/golden/make_oriented_rpn.py); the inputs are those of tests/rpn_cases.py, whose conditions tests/test_rpn_host.py asserts.
  1. anchor grid and inside flags, exact, for the two image shapes;
  2. the coder: encode and decode against rpn_ref, both clamps and the collapsed rectangle;
  3. targets + loss with the recorded sample indices: per-level losses and dense gradients against f22 in NCHW strides and in row strides, zero off the
     sampled anchors, the image without gts, two calls bit-identical;
  4. the sampler without injection: counts, membership, no duplicates, a seeded generator, no host synchronisation;
  5. proposals: kept index lists exact, boxes and scores close, against f22; with a min_bbox_size that removes boxes; the decode launch with one
     level cut by nms_pre and four kept whole;
  6. forward and loss_and_grads against the same three convolutions in torch on the CPU, fp32 and bf16.
Every bound is 4 x the error of the float32 CPU restatement against float64 (floor 1e-6), computed here; both numbers are recorded."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
import rpn_cases as RC
import rpn_ref as R
from conftest import record_parity
from mtp_amd import MODELS, ops
from mtp_amd.task_modules import AnchorGenerator, AssignResult, MidpointOffsetCoder, RandomSampler

pytestmark = pytest.mark.gpu
CASES = list(RC.SHAPES)
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


@pytest.fixture(scope="module")
def f22(golden):
    return golden("f22_oriented_rpn.npz")


def dev(a):
    """an op INPUT on the device, frozen"""
    return ARENA.frozen(ARENA.like(torch.as_tensor(np.ascontiguousarray(a))))


def err_of(a, ref):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a.astype(np.float64) - ref).max()) if ref.size else 0.0


def held(tag, out, ref64, ref32):
    """4 x the float32 CPU error of the restatement against float64, floor 1e-6"""
    err, e32 = err_of(out, ref64), err_of(ref32, ref64)
    record_parity("rpn", tag, err)
    record_parity("rpn", "rpn_ref_f32_cpu_" + tag, e32)
    assert tuple(out.shape) == ref64.shape and err < max(4 * e32, 1e-6), (tag, err, e32)


def make_head(in_channels=8, feat_channels=8, precision="fp32", proposal=None):
    return MODELS.build(dict(
        type="MTP_RD_OrientedRPNHead", in_channels=in_channels, feat_channels=feat_channels, precision=precision,
        anchor_generator=dict(type="mmdet.AnchorGenerator", scales=list(RC.SCALES), ratios=list(RC.RATIOS), strides=list(RC.STRIDES), use_box_type=True),
        bbox_coder=dict(type="MidpointOffsetCoder", angle_version="le90", target_means=list(RC.MEANS), target_stds=list(RC.STDS)),
        loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0), loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=RC.BETA, loss_weight=1.0),
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", iou_calculator=dict(type="mmrotate.RBbox2HBboxOverlaps2D"), **RC.ASSIGNER),
                       sampler=dict(type="RandomSampler", num=RC.NUM, pos_fraction=RC.POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=False),
                       allowed_border=0, pos_weight=-1, debug=False),
        test_cfg=dict(proposal or RC.PROPOSAL))).cuda()


def gt_instances(name):
    return [NS(rboxes=dev(g.reshape(-1, 5)), rlabels=torch.zeros(len(g), dtype=torch.int64, device="cuda")) for g in RC.case(name)[2]]


def recorded(f22, name):
    """the reference's choice: per image (pos_inds, neg_inds) into the anchors inside the image"""
    return [(f22["%s.image%d.pos_inds" % (name, b)], f22["%s.image%d.neg_inds" % (name, b)]) for b in range(RC.BATCH)]


def sampled(f22, name):
    inside = np.nonzero(RC.anchors(name)[1])[0]
    q = ["%s.image%d." % (name, b) for b in range(RC.BATCH)]
    return [inside[f22[p + "pos_inds"]] for p in q], [f22[p + "pos_gt"] for p in q], [inside[f22[p + "neg_inds"]] for p in q]


# ------------------------------------------------------------------------------------------------------------------- 1. anchors
@pytest.mark.parametrize("name", CASES)
def test_anchor_grid_and_inside_flags_exact(name):
    img, pad, _ = RC.SHAPES[name]
    priors, inside, sizes = RC.anchors(name)
    gen = AnchorGenerator(strides=list(RC.STRIDES), ratios=list(RC.RATIOS), scales=list(RC.SCALES))
    first = 0
    for (H, W), s, base in zip(sizes, gen.strides, gen.base_anchors):
        n = H * W * RC.A
        p, f = ARENA.empty(n, 4), ARENA.empty(n, dtype=torch.uint8)
        ops.rpn_anchors(dev(base), H, W, s, pad, img, 0, p, f)
        assert np.array_equal(p.cpu().numpy(), priors[first:first + n].astype(np.float32)) and np.array_equal(f.cpu().numpy().astype(bool), inside[first:first + n])
        ops.rpn_anchors(dev(base), H, W, s, pad, img, -1, p, f)      # a negative border: the valid flags alone
        assert np.array_equal(f.cpu().numpy().astype(bool), R.inside_flags(priors[first:first + n], RC.A, H, W, s, pad, img, -1))
        first += n
    assert first == len(priors)
    got = gen.priors_and_flags(sizes, pad, img, 0, "cuda")
    assert gen.priors_and_flags(sizes, pad, img, 0, "cuda") is got      # cached per key
    assert np.array_equal(torch.cat([p for p, _ in got]).cpu().numpy(), priors.astype(np.float32))
    assert np.array_equal(torch.cat([f for _, f in got]).cpu().numpy().astype(bool), inside)
    assert np.array_equal(torch.cat(gen.grid_priors(sizes, device="cuda")).cpu().numpy(), priors.astype(np.float32))
    valid = torch.cat(gen.valid_flags(sizes, pad, device="cuda")).cpu().numpy()
    assert valid.dtype == bool and np.array_equal(valid, np.concatenate([R.inside_flags(priors[:0], RC.A, H, W, (s, s), pad, pad, -1) for (H, W), s in zip(sizes, RC.STRIDES)]))


# ------------------------------------------------------------------------------------------------------------------- 2. the coder
def coder_inputs(n, seed):
    rng = np.random.default_rng(seed)
    priors, inside, _ = RC.anchors("sq128")
    p = priors[inside][rng.integers(0, int(inside.sum()), n)].astype(np.float32)
    c = np.stack([(p[:, 0] + p[:, 2]) / 2, (p[:, 1] + p[:, 3]) / 2], 1)
    g = np.concatenate([c + rng.uniform(-6, 6, (n, 2)), rng.uniform(8, 60, (n, 2)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1).astype(np.float32)
    keep = np.array([RC.corner_condition(g[i:i + 1]) for i in range(n)])      # (the 0.1 cut is decided in float64: stay clear of it)
    return p[keep], g[keep]


@pytest.mark.parametrize("n", [1, 65, 600])
def test_coder_encode(n):
    p, g = coder_inputs(n, 10 + n)
    coder = MidpointOffsetCoder(target_means=RC.MEANS, target_stds=RC.STDS)
    out = coder.encode(dev(p), dev(g))
    held("encode_%d" % n, out, R.encode(p, g, RC.MEANS, RC.STDS), R.encode(p, g, RC.MEANS, RC.STDS, R.F32))
    other = ((0.1, -0.2, 0.3, 0.0, 0.05, -0.05), (0.5, 0.5, 0.25, 0.25, 0.3, 0.7))      # means and stds that are not the identity
    out = MidpointOffsetCoder(*other).encode(dev(p), dev(g))
    held("encode_means_%d" % n, out, R.encode(p, g, *other), R.encode(p, g, *other, R.F32))
    assert tuple(coder.encode(torch.zeros(0, 4, device="cuda"), torch.zeros(0, 5, device="cuda")).shape) == (0, 6)


@pytest.mark.parametrize("n", [1, 65, 600])
def test_coder_decode(n):
    rng = np.random.default_rng(20 + n)
    p = coder_inputs(n, 30 + n)[0]
    n = len(p)
    d = rng.normal(0, 0.4, (n, 6))
    d[:, 4:] = rng.uniform(-0.95, 0.95, (n, 2))
    if n > 20:      # both clamps: sizes beyond exp(+-|log(16 / 1000)|), midpoint offsets beyond +-0.5 on one side
        d[:6, 2], d[:6, 3] = [9, -9, 5, 4.2, -4.2, 0], [0, 9, -9, -5, 4.2, -4.2]
        d[6:12, 4], d[6:12, 5] = [1.5, -1.5, 3, 0.2, -0.2, 1.01], [0.3, 0.1, -0.4, 2.0, -2.0, 0.0]
    d = d.astype(np.float32)
    ref = R.decode(p, d, RC.MEANS, RC.STDS)
    fine = (np.abs(ref[:, 2] - ref[:, 3]) > RC.SHAPE_GAP * ref[:, 2]) & (np.abs(np.abs(ref[:, 4]) - np.pi / 2) > RC.SHAPE_GAP)      # as rpn_cases has it
    p, d, ref = p[fine], d[fine], ref[fine]
    assert fine[:12].sum() >= 8 or n <= 20      # the clamped rows are among what is compared
    coder = MidpointOffsetCoder(target_means=RC.MEANS, target_stds=RC.STDS)
    out = coder.decode(dev(p), dev(d), max_shape=(128, 128))
    held("decode_%d" % n, out, ref, R.decode(p, d, RC.MEANS, RC.STDS, R.F32))
    assert (out[:, 2] >= out[:, 3]).all() and (out[:, 4] >= -np.pi / 2).all() and (out[:, 4] < np.pi / 2).all()


def test_coder_decode_collapsed_rectangle():
    """da = +-0.5 with db = -+0.5 (clamped or exact): the rectangle is a segment, h = 0 exactly, nothing is NaN, and the proposal is not valid"""
    p = np.array([[10, 20, 42, 52], [0, 0, 22.627417, 45.254833], [100.5, 60.25, 164.5, 124.25], [3, 4, 35, 36]], np.float32)
    d = np.array([[0.1, 0.2, 0.3, -0.2, 1.0, -1.0], [0, 0, 0, 0, -1.0, 1.0], [0.5, -0.5, 1, 1, 7.0, -9.0], [0, 0, -5, 5, -1.0, 2.5]], np.float32)
    out = MidpointOffsetCoder(target_means=RC.MEANS, target_stds=RC.STDS).decode(dev(p), dev(d))
    ref = R.decode(p, d, RC.MEANS, RC.STDS)
    assert torch.isfinite(out).all() and (out[:, 3] == 0).all() and (out[:, 2] > 0).all() and (ref[:, 3] == 0).all()
    held("decode_collapsed", out, ref, R.decode(p, d, RC.MEANS, RC.STDS, R.F32))
    # the same through the proposal launch: one level of 2 x 2 cells, one anchor each, the four priors above
    cls, reg = dev(np.zeros((1, 1, 2, 2), np.float32)), dev(d.T.reshape(1, 6, 2, 2))
    o = ops.rpn_proposals([ops.rpn_map_nchw(cls)], [ops.rpn_map_nchw(reg)], [(2, 2)], 1, dev(p), dev(np.arange(4)[None]), [4], RC.MEANS, RC.STDS, 0.0)
    assert not o[4].any() and torch.isfinite(o[1]).all() and torch.isfinite(o[2]).all() and torch.equal(o[1][0], out) and (o[0] == 0.5).all()


# ------------------------------------------------------------------------------------------------------------------- 3. targets and loss
def rows_of(maps_cls, maps_reg):
    """the NCHW maps of all levels as one (rows, 24) buffer in the engines' row layout, and each level's first row"""
    blocks, row0, rows = [], [], 0
    for c, r in zip(maps_cls, maps_reg):
        N, A, H, W = c.shape
        m = np.concatenate([c, r, np.zeros((N, 24 - 7 * A, H, W), np.float32)], 1)
        blocks.append(np.transpose(m, (0, 2, 3, 1)).reshape(N * H * W, 24))
        row0.append(rows)
        rows += N * H * W
    return np.concatenate(blocks), row0


@pytest.mark.parametrize("name", CASES)
def test_targets_and_loss_vs_f22(f22, name):
    cls, reg, gts = RC.case(name)
    priors, _, sizes = RC.anchors(name)
    L = len(sizes)
    pos, pgt, neg = sampled(f22, name)
    ref32 = R.loss(cls, reg, sizes, RC.A, priors, gts, pos, pgt, neg, RC.MEANS, RC.STDS, RC.BETA, dtype=R.F32)
    head = make_head()
    tc, tr = [dev(m) for m in cls], [dev(m) for m in reg]
    # --- NCHW strides, through the head: assigner, sampler with the reference's choice, the two launches
    losses, dcls, dreg = head.loss_by_feat(tc, tr, gt_instances(name), RC.metas(name), sample_inds=recorded(f22, name), return_grads=True)
    lc, lb = torch.stack(losses["loss_rpn_cls"]), torch.stack(losses["loss_rpn_bbox"])
    held(name + "_loss_cls", lc, f22[name + ".loss_cls"], ref32[0])
    held(name + "_loss_bbox", lb, f22[name + ".loss_bbox"], ref32[1])
    for l in range(L):
        q = "%s.level%d." % (name, l)
        held("%s_dcls_%d" % (name, l), dcls[l], f22[q + "dcls"], ref32[2][l])
        held("%s_dreg_%d" % (name, l), dreg[l], f22[q + "dreg"], ref32[3][l])
        # exactly zero off the sampled anchors (and the reference's gradient vanishes nowhere on them)
        assert not dcls[l].cpu().numpy()[f22[q + "dcls"] == 0].any() and not dreg[l].cpu().numpy()[f22[q + "dreg"] == 0].any()
        assert int((f22[q + "dcls"] != 0).sum()) == int(f22[q + "label_weights"].sum()) and int((f22[q + "dreg"] != 0).sum()) == int(f22[q + "bbox_weights"].sum())
    assert int(sum(f22["%s.level%d.label_weights" % (name, l)].sum() for l in range(L))) == RC.BATCH * RC.NUM
    if name == "pad160":      # the image without gts: 16 negatives, no box loss, no box gradient
        assert len(pos[1]) == 0 and len(neg[1]) == RC.NUM and not any(d[1].any() for d in dreg) and sum(int((d[1] != 0).sum()) for d in dcls) == RC.NUM
    # --- two calls: the same bits
    again = head.loss_by_feat(tc, tr, gt_instances(name), RC.metas(name), sample_inds=recorded(f22, name), return_grads=True)
    assert torch.equal(torch.stack(again[0]["loss_rpn_cls"]), lc) and torch.equal(torch.stack(again[0]["loss_rpn_bbox"]), lb)
    assert all(torch.equal(a, b) for a, b in zip(again[1] + again[2], dcls + dreg))
    # --- row strides: the same sample lists on one (rows, 24) buffer, the gradient buffer in the same layout; the same bits as NCHW
    flat, gts_all, samples, sample_gt, n_pos, n_neg = head.get_samples(sizes, gt_instances(name), RC.metas(name), "cuda", sample_inds=recorded(f22, name))
    assert n_pos.tolist() == [len(p) for p in pos] and n_neg.tolist() == [len(n) for n in neg]
    for b in range(RC.BATCH):
        assert samples[b, :len(pos[b]) + len(neg[b])].tolist() == list(pos[b]) + list(neg[b])
    rows, row0 = rows_of(cls, reg)
    buf, grad = dev(rows), ARENA.zeros(*rows.shape)
    mc = [ops.rpn_map_rows(buf, H, W, 0, r) for (H, W), r in zip(sizes, row0)]
    mr = [ops.rpn_map_rows(buf, H, W, RC.A, r) for (H, W), r in zip(sizes, row0)]
    gc, gr = [(grad,) + m[1:] for m in mc], [(grad,) + m[1:] for m in mr]
    lc2, lb2 = ops.rpn_loss(mc, mr, sizes, RC.A, flat, gts_all, samples, sample_gt, n_pos, n_neg, RC.MEANS, RC.STDS, RC.BETA, 1.0, 1.0, gc, gr,
                            ARENA.empty(L), ARENA.empty(L))
    assert torch.equal(lc2, lc) and torch.equal(lb2, lb)
    want, _ = rows_of([d.cpu().numpy() for d in dcls], [d.cpu().numpy() for d in dreg])
    assert np.array_equal(grad.cpu().numpy(), want)
    # --- loss weights scale losses and gradients; without gradient maps the losses are the same
    lc3, lb3 = ops.rpn_loss(mc, mr, sizes, RC.A, flat, gts_all, samples, sample_gt, n_pos, n_neg, RC.MEANS, RC.STDS, RC.BETA, 2.0, 0.5)
    assert torch.allclose(lc3, 2 * lc, rtol=1e-6, atol=0) and torch.allclose(lb3, 0.5 * lb, rtol=1e-6, atol=0)


def test_loss_refuses_what_it_cannot_address():
    cls, reg, _ = RC.case("sq128")
    priors, _, sizes = RC.anchors("sq128")
    tc, tr = [dev(m) for m in cls], [dev(m) for m in reg]
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")      # noqa: E731
    args = (dev(priors.astype(np.float32)), torch.zeros(0, 5, device="cuda"), i64(2, 16), i64(2, 16), i64(2), i64(2), RC.MEANS, RC.STDS, RC.BETA)
    mc, mr = [ops.rpn_map_nchw(m) for m in tc], [ops.rpn_map_nchw(m) for m in tr]
    lc, lb = ops.rpn_loss(mc, mr, sizes, RC.A, *args)      # no samples at all: avg_factor 0, zero losses, nothing divided by zero
    assert not lc.any() and not lb.any()
    with pytest.raises(ValueError):      # a map shorter than its strides say
        ops.rpn_loss([(tc[1],) + mc[0][1:]] + mc[1:], mr, sizes, RC.A, *args)
    with pytest.raises(ValueError):      # priors that are not the levels' anchors
        ops.rpn_loss(mc, mr, sizes, RC.A, args[0][:-3].contiguous(), *args[1:])
    with pytest.raises(ValueError):
        ops.rpn_loss(mc, mr, sizes, RC.A, *args, dcls=[(torch.zeros_like(m),) + ops.rpn_map_nchw(m)[1:] for m in tc])
    # indices out of range are ignored on the device, not followed
    bad = i64(2, 16)
    bad[0, :4] = torch.tensor([-1, len(priors), 1 << 40, 5], device="cuda")
    one = torch.tensor([4, 0], device="cuda")
    lc, lb = ops.rpn_loss(mc, mr, sizes, RC.A, args[0], args[1], bad, i64(2, 16) + 7, one, i64(2), *args[6:])
    assert float(lb.abs().sum()) == 0 and float(lc[0]) > 0 and not lc[1:].any()      # anchor 5 alone counts; its gt index 7 names no gt


# ------------------------------------------------------------------------------------------------------------------- 4. the sampler
def test_sampler_properties_without_a_host_synchronisation():
    rng = np.random.default_rng(4)
    gt_inds = np.concatenate([rng.integers(1, 7, 40), np.zeros(1800, np.int64), -np.ones(44, np.int64)])
    gt_inds = torch.as_tensor(rng.permutation(gt_inds)).cuda()
    s = RandomSampler(RC.NUM, RC.POS_FRACTION, neg_pos_ub=-1, add_gt_as_proposals=False)
    gens = [torch.Generator(device="cuda").manual_seed(11) for _ in range(2)] + [torch.Generator(device="cuda").manual_seed(12)]
    few = torch.as_tensor(np.array([3, 0, 0, -1, 0, 1, 0, 0], np.int64)).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        runs = [s.sample(AssignResult(6, gt_inds, None, None), generator=g) for g in gens]
        small = s.sample(AssignResult(3, few, None, None), generator=gens[0])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    a, b, c = runs
    assert torch.equal(a.inds, b.inds) and torch.equal(a.gt_inds, b.gt_inds) and not torch.equal(a.inds, c.inds)      # the generator decides
    for r in runs:
        assert int(r.n_pos) == int(RC.NUM * RC.POS_FRACTION) and int(r.n_neg) == RC.NUM - int(r.n_pos) and tuple(r.inds.shape) == (RC.NUM,)
        assert (gt_inds[r.pos_inds] > 0).all() and (gt_inds[r.neg_inds] == 0).all() and len(set(r.inds.tolist())) == RC.NUM
        assert torch.equal(r.pos_assigned_gt_inds, gt_inds[r.pos_inds] - 1) and (r.gt_inds[int(r.n_pos):] == -1).all()
    # fewer candidates than asked for: all 2 positives, all 5 negatives
    assert int(small.n_pos) == 2 and int(small.n_neg) == 5 and sorted(small.pos_inds.tolist()) == [0, 5] and sorted(small.neg_inds.tolist()) == [1, 2, 4, 6, 7]
    # in distribution the reference's choice: over many draws every positive is taken about equally often
    hits = torch.zeros_like(gt_inds)
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(200):
        hits[s.sample(AssignResult(6, gt_inds, None, None), generator=g).pos_inds] += 1
    h = hits[gt_inds > 0].float()
    assert int(hits[gt_inds <= 0].sum()) == 0 and float(h.sum()) == 200 * 8 and float(h.min()) >= 15 and float(h.max()) <= 70      # mean 40, sd 5.7


# ------------------------------------------------------------------------------------------------------------------- 5. proposals
@pytest.mark.parametrize("tag,min_size", [("prop", 0), ("prop_min", RC.MIN_SIZE)])
@pytest.mark.parametrize("name", CASES)
def test_proposals_vs_f22(f22, name, tag, min_size):
    cls, reg, _ = RC.case(name)
    priors, _, sizes = RC.anchors(name)
    head = make_head(proposal=dict(RC.PROPOSAL, min_bbox_size=min_size))
    res = head.predict_by_feat([dev(m) for m in cls], [dev(m) for m in reg], batch_img_metas=RC.metas(name))
    again = head.predict_by_feat([dev(m) for m in cls], [dev(m) for m in reg], batch_img_metas=RC.metas(name), cfg=dict(RC.PROPOSAL, min_bbox_size=min_size))
    for b, r in enumerate(res):
        q = "%s.%s.image%d." % (name, tag, b)
        cb, rb = [m[b] for m in cls], [m[b] for m in reg]
        assert r.keep.tolist() == f22[q + "keep"].tolist()      # exact, in order
        top = R.topk_per_level(cb, RC.PROPOSAL["nms_pre"])
        sc32, rb32 = R.decode_kept(cb, rb, priors, sizes, RC.A, top, RC.MEANS, RC.STDS, R.F32)[:2]
        held("%s_%s_boxes_%d" % (name, tag, b), r.bboxes, f22[q + "bboxes"], rb32[f22[q + "keep"]])
        held("%s_%s_scores_%d" % (name, tag, b), r.scores, f22[q + "scores"], sc32[f22[q + "keep"]])
        assert r.labels.dtype == torch.int64 and not r.labels.any() and len(r.labels) == len(r.scores) <= RC.PROPOSAL["max_per_img"]
        assert (r.bboxes[:, 2] > min_size).all() and (r.bboxes[:, 3] > min_size).all()
        assert torch.equal(again[b].keep, r.keep) and torch.equal(again[b].bboxes, r.bboxes) and torch.equal(again[b].scores, r.scores)


def test_proposal_decode_one_level_cut_four_whole():
    """nms_pre = 1000: level 0 (3072 anchors) is cut, the four others are kept whole.  The decode launch alone: per level the kept SET is the
    reference's (the cut clears SCORE_GAP, asserted here from float64 alone), every entry is the decode of the anchor it names."""
    name, nms_pre = "sq128", 1000
    cls, reg, _ = RC.case(name)
    priors, _, sizes = RC.anchors(name)
    counts = [min(nms_pre, h * w * RC.A) for h, w in sizes]
    assert counts == [1000, 768, 192, 48, 12]
    tc, tr = [dev(m) for m in cls], [dev(m) for m in reg]
    keep = torch.cat([torch.sort(m.permute(0, 2, 3, 1).reshape(RC.BATCH, -1), dim=1, descending=True, stable=True)[1][:, :k] for m, k in zip(tc, counts)], 1)
    keep = ARENA.frozen(keep.contiguous())
    T = sum(counts)
    out = (ARENA.empty(RC.BATCH, T), ARENA.empty(RC.BATCH, T, 5), ARENA.empty(RC.BATCH, T, 4), ARENA.empty(RC.BATCH, T, dtype=torch.int64),
           ARENA.empty(RC.BATCH, T, dtype=torch.uint8))
    ops.rpn_proposals([ops.rpn_map_nchw(m) for m in tc], [ops.rpn_map_nchw(m) for m in tr], sizes, RC.A, dev(priors.astype(np.float32)), keep, counts,
                      RC.MEANS, RC.STDS, float(RC.MIN_SIZE), out)
    scores, rboxes, hboxes, level_ids, valid = out
    assert level_ids[0].tolist() == [l for l, k in enumerate(counts) for _ in range(k)] and torch.equal(level_ids[0], level_ids[1])
    for b in range(RC.BATCH):
        cb, rb = [m[b] for m in cls], [m[b] for m in reg]
        z0 = np.sort(np.transpose(cb[0], (1, 2, 0)).reshape(-1).astype(np.float64))[::-1]
        assert 1 / (1 + np.exp(-z0[nms_pre - 1])) - 1 / (1 + np.exp(-z0[nms_pre])) > RC.SCORE_GAP
        first, got = 0, []
        for l, k in enumerate(counts):
            mine = keep[b, first:first + k].cpu().numpy()
            assert sorted(mine.tolist()) == sorted(R.topk_per_level([cb[l]], nms_pre)[0].tolist())
            got.append(mine)
            first += k
        sc, rbx, hb, ids = R.decode_kept(cb, rb, priors, sizes, RC.A, got, RC.MEANS, RC.STDS)
        sc32, rb32, hb32, _ = R.decode_kept(cb, rb, priors, sizes, RC.A, got, RC.MEANS, RC.STDS, R.F32)
        sure = (np.abs(rbx[:, 2] - rbx[:, 3]) > RC.SHAPE_GAP * rbx[:, 2]) & (np.abs(np.abs(rbx[:, 4]) - np.pi / 2) > RC.SHAPE_GAP)      # as rpn_cases has it
        assert sure.mean() > 0.99
        held("cut_scores_%d" % b, scores[b], sc, sc32)
        held("cut_rboxes_%d" % b, rboxes[b][torch.as_tensor(sure).cuda()], rbx[sure], rb32[sure])
        held("cut_hboxes_%d" % b, hboxes[b][torch.as_tensor(sure).cuda()], hb[sure], hb32[sure])
        clear = (np.abs(rbx[:, 2] - RC.MIN_SIZE) > RC.SHAPE_GAP) & (np.abs(rbx[:, 3] - RC.MIN_SIZE) > RC.SHAPE_GAP)
        want = (rbx[:, 2] > RC.MIN_SIZE) & (rbx[:, 3] > RC.MIN_SIZE)
        assert np.array_equal(valid[b].cpu().numpy().astype(bool)[clear], want[clear]) and 0 < want.sum() < len(want)


# ------------------------------------------------------------------------------------------------------------------- 6. the convolutions
def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def composition(feats, w, dcls_of, rounding, dtype):
    """the three convolutions in torch on the CPU in `dtype` -> (cls maps, reg maps, gradients of the parameters, gradients of the inputs) for the
    loss gradient dcls_of(cls, reg) -> (dcls, dreg).  rounding: the operands of every GEMM the engine runs in bf16 are rounded to bf16 -- inputs,
    weights, the 3x3 convolution's output, and in the backward the loss gradient and the gradient behind the ReLU."""
    r = (lambda t: t + (bf16_round(t) - t).detach()) if rounding else (lambda t: t)
    rg = (lambda t: t.register_hook(bf16_round) and t) if rounding else (lambda t: t)
    P = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in w.items()}
    xs = [f.detach().cpu().to(dtype).requires_grad_() for f in feats]
    cls, reg = [], []
    for x in xs:
        z = rg(r(F.conv2d(r(x), r(P["rpn_conv.weight"]), P["rpn_conv.bias"], padding=1)))
        y = F.relu(z)
        out = rg(torch.cat([F.conv2d(y, r(P["rpn_cls.weight"]), P["rpn_cls.bias"]), F.conv2d(y, r(P["rpn_reg.weight"]), P["rpn_reg.bias"])], 1))
        cls.append(out[:, :RC.A])
        reg.append(out[:, RC.A:])
    dcls, dreg = dcls_of([c.detach() for c in cls], [g.detach() for g in reg])
    grads = torch.autograd.grad(cls + reg, list(P.values()) + xs, [torch.as_tensor(d).to(dtype) for d in dcls + dreg])
    return [c.detach() for c in cls], [g.detach() for g in reg], dict(zip(P, grads[:len(P)])), list(grads[len(P):])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_and_loss_and_grads_vs_torch(f22, precision):
    name, Cin, Cf = "sq128", 16, 32
    _, _, gts = RC.case(name)
    priors, _, sizes = RC.anchors(name)
    pos, pgt, neg = sampled(f22, name)
    torch.manual_seed(6)
    head = make_head(Cin, Cf, precision)
    for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
        torch.nn.init.normal_(m.weight, 0.0, 0.08)
        torch.nn.init.normal_(m.bias, 0.0, 0.2)
    feats = [torch.randn(RC.BATCH, Cin, H, W).cuda() for H, W in sizes]
    w = {k: v.detach() for k, v in head.named_parameters()}

    def dcls_of(cls, reg):      # the loss gradient of the maps at hand, from the float64 restatement
        out = R.loss([c.numpy() for c in cls], [g.numpy() for g in reg], sizes, RC.A, priors, gts, pos, pgt, neg, RC.MEANS, RC.STDS, RC.BETA)
        return out[2], out[3]
    truth = composition(feats, w, dcls_of, False, torch.float64)
    yard = composition(feats, w, dcls_of, precision == "bf16", torch.float32)
    cls, reg = head(feats)
    losses, G, dx = head.loss_and_grads(feats, gt_instances(name), RC.metas(name), sample_inds=recorded(f22, name))
    assert list(G) == [k for k, _ in head.named_parameters()] and all(p.grad is None for p in head.parameters())
    ref_l = R.loss([c.numpy() for c in truth[0]], [g.numpy() for g in truth[1]], sizes, RC.A, priors, gts, pos, pgt, neg, RC.MEANS, RC.STDS, RC.BETA)
    yard_l = R.loss([c.numpy() for c in yard[0]], [g.numpy() for g in yard[1]], sizes, RC.A, priors, gts, pos, pgt, neg, RC.MEANS, RC.STDS, RC.BETA, dtype=R.F32)
    tag = "head_%s_" % precision
    held(tag + "loss_cls", torch.stack(losses["loss_rpn_cls"]), ref_l[0], yard_l[0])
    held(tag + "loss_bbox", torch.stack(losses["loss_rpn_bbox"]), ref_l[1], yard_l[1])
    for l in range(len(sizes)):
        held("%scls_%d" % (tag, l), cls[l], truth[0][l].numpy(), yard[0][l].numpy())
        held("%sreg_%d" % (tag, l), reg[l], truth[1][l].numpy(), yard[1][l].numpy())
        held("%sdx_%d" % (tag, l), dx[l], truth[3][l].numpy(), yard[3][l].numpy())
    for k in G:
        held(tag + k, G[k], truth[2][k].numpy(), yard[2][k].numpy())
    # one run of the convolutions for the loss and the proposals
    l2, res = head.loss_and_predict(feats, gt_instances(name), RC.metas(name), sample_inds=recorded(f22, name))
    assert torch.equal(torch.stack(l2["loss_rpn_cls"]), torch.stack(losses["loss_rpn_cls"])) and len(res) == RC.BATCH
    alone = head.predict_by_feat(cls, reg, batch_img_metas=RC.metas(name))
    for a, r in zip(alone, res):
        assert torch.equal(a.keep, r.keep) and torch.equal(a.bboxes, r.bboxes) and torch.equal(a.scores, r.scores) and 0 < len(r.scores) <= RC.PROPOSAL["max_per_img"]
