"""GPU: the box operators of csrc/box_ops.hip through mtp_amd.ops_box and mtp_amd.task_modules, every buffer out of a guard.Arena (poisoned outputs, guards
on both sides, frozen inputs, the wrappers' own workspaces included).  The reference is tests/box_ref.py in float64; the inputs are those of
tests/box_cases.py, whose conditions tests/test_box_host.py asserts.
  * IoU, both kinds: (M, N) in {(1,1), (3,65), (65,3), (130,257)}, 'iou' and 'iof', pairwise and aligned; the regimes (zero-area boxes, boxes that touch
    along an edge, one box inside another; rotated: the analytic cases, a 4-px box at cx = 1000, two angles 1e-4 rad apart).  The bound of each case is
    4 x the error of box_ref run in float32 on the CPU against float64 (floor 1e-6), computed here, both numbers recorded.  On the NMS input sets the
    error also stays below a quarter of the set's gap, for every set the NMS tests use.
  * NMS, both kinds: exact index lists at every threshold for n in {1, 2, 63, 64, 65, 128, 129} (rotated: n <= 65), the chain set (n = 2049), all
    and at n = 4225, where the scan's lanes stride twice over the column blocks), all identical, all disjoint, identical under different group ids,
    max_num, score_threshold, the constructed tie, batched_nms, two calls.
  * assignment: fixture f21 (the reference's own runs) on the device; (K, N) in {(1,1), (3,65), (65,64), (65,1000)} x three calculators x five
    configurations; K = 300 (more gts than one LDS tile, a duplicate pair and low-quality matches across the boundary); duplicate gts, duplicate priors,
    a gt that overlaps nothing at min_pos_iou = 0, K = 0, N = 0, two calls.  gt_inds and labels exact, max_overlaps within the IoU bound."""
import math

import numpy as np
import pytest
import torch

import box_cases as C
import box_ref as R
import guard
from conftest import record_parity
from mtp_amd import TASK_UTILS, ops
from mtp_amd.ops_box import batched_nms, bbox_overlaps, box_iou_rotated, nms, nms_rotated
from mtp_amd.task_modules import MaxIoUAssigner

pytestmark = pytest.mark.gpu
I64 = torch.int64
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
    return ARENA.frozen(ARENA.like(torch.as_tensor(a)))


def err_of(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) if ref.size else 0.0


def check_iou(out, ref64, ref32, tag):
    """4 x the float32 CPU error of box_ref against float64, floor 1e-6"""
    err, e32 = err_of(out.cpu().numpy(), ref64), err_of(ref32, ref64)
    record_parity("box_ops", "iou_" + tag, err)
    record_parity("box_ops", "iou_box_ref_f32_cpu_" + tag, e32)
    assert tuple(out.shape) == ref64.shape and err < max(4 * e32, 1e-6), (tag, err, e32)
    return err


def ref_iou(b1, b2, rotated, mode, aligned, dtype):
    return R.box_iou_rotated(b1, b2, mode, aligned, dtype=dtype) if rotated else R.bbox_overlaps(b1, b2, mode, aligned, dtype=dtype)


def hip_iou(b1, b2, rotated, mode, aligned):
    return box_iou_rotated(dev(b1), dev(b2), mode, aligned) if rotated else bbox_overlaps(dev(b1), dev(b2), mode, aligned)


# ------------------------------------------------------------------------------------------------------------------- IoU
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("M,N", [(1, 1), (3, 65), (65, 3), (130, 257)])
def test_iou_vs_float64(M, N, rotated):
    rng = np.random.default_rng(7)
    b1, b2 = C.rand_boxes(M, rng, rotated), C.rand_boxes(N, rng, rotated)
    m = min(M, N)
    b2[:m:2] = b1[:m:2] + C.f32(rng.uniform(-2, 2, b1[:m:2].shape) * ([1, 1, 1, 1, 0.02] if rotated else [1] * 4))      # high overlaps too
    for mode in ("iou", "iof"):
        tag = "%s_%dx%d_%s" % ("rot" if rotated else "box", M, N, mode)
        check_iou(hip_iou(b1, b2, rotated, mode, False), ref_iou(b1, b2, rotated, mode, False, R.F64), ref_iou(b1, b2, rotated, mode, False, R.F32), tag)
        check_iou(hip_iou(b1[:m], b2[:m], rotated, mode, True), ref_iou(b1[:m], b2[:m], rotated, mode, True, R.F64),
                  ref_iou(b1[:m], b2[:m], rotated, mode, True, R.F32), tag + "_aligned")


BOX_REGIMES = {      # name -> (boxes1, boxes2), aligned pairs
    "zero_area": ([[10, 10, 10, 30], [5, 5, 5, 5], [0, 0, 20, 20]], [[0, 0, 20, 40], [5, 5, 5, 5], [8, 3, 8, 9]]),
    "touching": ([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]], [[10, 0, 20, 10], [0, 10, 10, 25], [10, 10, 20, 20]]),
    "inside": ([[0, 0, 10, 10], [4, 4, 6, 6], [100, 50, 164, 114]], [[4, 4, 6, 6], [0, 0, 10, 10], [100.5, 50.25, 108.5, 58.25]]),
}
_U, _B, _T = [0, 0, 1, 1, 0], [30, 40, 20, 8, 0.7], 0.3
ROT_REGIMES = {
    "zero_area": ([[10, 10, 0, 30, 0.3], [5, 5, 0, 0, 0], [10, 10, 20, 20, 1.0]], [[10, 10, 20, 40, 0.1], [5, 5, 0, 0, 0], [8, 9, 1e-8, 1e-8, 0.5]]),
    "touching": ([[5, 5, 10, 10, 0], [5, 5, 10, 10, 0], [0, 0, 10, 10, _T]],
                 [[15, 5, 10, 10, 0], [15, 15, 10, 10, 0], [10 * math.cos(_T), 10 * math.sin(_T), 10, 10, _T]]),
    "inside": ([[5, 5, 2, 2, 0.3], [5, 5, 10, 10, 0.3], [50, 60, 40, 30, -1.0]], [[5, 5, 10, 10, 0.3], [5, 5, 2, 2, 0.3], [51, 59, 6, 5, 0.4]]),
    "unit_square_45": ([_U], [[0, 0, 1, 1, math.pi / 4]]),
    "self_half_turn_and_swapped": ([_B, _B], [[30, 40, 20, 8, 0.7 + math.pi], [30, 40, 8, 20, 0.7 + math.pi / 2]]),
    "shifted_along_axis": ([[100, 100, 10, 10, _T]] * 10, [[100 + d * math.cos(_T), 100 + d * math.sin(_T), 10, 10, _T] for d in range(10)]),
    "four_px_at_1000": ([[1000, 1000, 4, 4, 0.2], [1000.25, 999.5, 4, 4, -0.4]], [[1001, 1000.5, 4, 4, 0.5], [1001.5, 1000, 4, 3, 1.2]]),
    "angles_1e-4_apart": ([[60, 70, 50, 20, 0.5], [60, 70, 50, 20, -1.2]], [[60, 70, 50, 20, 0.5001], [60, 70, 50, 20, -1.2001]]),
}
ANALYTIC = {"unit_square_45": [1 / math.sqrt(2)], "self_half_turn_and_swapped": [1.0, 1.0], "shifted_along_axis": [(10 - d) / (10 + d) for d in range(10)]}


@pytest.mark.parametrize("rotated,name", [(False, k) for k in BOX_REGIMES] + [(True, k) for k in ROT_REGIMES])
def test_iou_regimes(rotated, name):
    b1, b2 = (C.f32(b) for b in (ROT_REGIMES if rotated else BOX_REGIMES)[name])
    for mode in ("iou", "iof"):
        r64 = ref_iou(b1, b2, rotated, mode, True, R.F64)
        out = hip_iou(b1, b2, rotated, mode, True)
        check_iou(out, r64, ref_iou(b1, b2, rotated, mode, True, R.F32), "%s_%s_%s" % ("rot" if rotated else "box", name, mode))
        pair = hip_iou(b1, b2, rotated, mode, False)                      # the pairwise form holds the aligned one on its diagonal, bit for bit
        assert torch.equal(pair.diagonal(), out)
        if name == "zero_area" or (name == "touching" and not rotated):
            assert float(out.abs().max()) == 0.0
        if mode == "iou" and name in ANALYTIC:
            assert err_of(out.cpu().numpy(), np.asarray(ANALYTIC[name])) < 1e-5      # (the inputs themselves are rounded to float32: 7.6e-6 px at 100)


@pytest.mark.parametrize("rotated", [False, True])
def test_iou_error_on_the_nms_sets_is_below_a_quarter_of_their_gap(rotated):
    sets = [("n%d" % n, ("rand", rotated, n), C.nms_set(n, rotated)[0], C.NMS_GAP) for n in C.NMS_SIZES[rotated]]      # every set the NMS tests use
    gap = min(C.chain_margins(rotated).values())
    sets += [("chain", ("chain", rotated, C.CHAIN_N), C.chain_set(rotated)[0], gap), ("chain_wide", ("chain", rotated, C.CHAIN_N_WIDE), C.chain_set(rotated, C.CHAIN_N_WIDE)[0], gap)]
    for tag, key, boxes, gap in sets:
        err = err_of(hip_iou(boxes, boxes, rotated, "iou", False).cpu().numpy(), iou64_of(key, boxes, rotated))
        record_parity("box_ops", "iou_nms_set_%s_%s" % ("rot" if rotated else "box", tag), err)
        assert err < gap / 4, (tag, err, gap)


# ------------------------------------------------------------------------------------------------------------------- NMS
_IOU64 = {}


def iou64_of(key, boxes, rotated):
    """the float64 matrix of an input set, computed once and shared"""
    if key not in _IOU64:
        _IOU64[key] = C.iou64(boxes, boxes, rotated)
    return _IOU64[key]


def hip_nms(boxes, scores, thr, rotated, labels=None, **kw):
    if rotated:
        dets, inds = nms_rotated(dev(boxes), dev(scores), thr, None if labels is None else dev(labels))
    else:
        assert labels is None
        dets, inds = nms(dev(boxes), dev(scores), thr, **kw)
    assert inds.dtype == I64 and dets.shape == (inds.numel(), boxes.shape[1] + 1)
    k = inds.cpu()
    assert torch.equal(dets.cpu(), torch.cat([torch.from_numpy(boxes)[k], torch.from_numpy(scores)[k, None]], 1))
    return k.tolist()


@pytest.mark.parametrize("rotated,n", [(r, n) for r in (False, True) for n in C.NMS_SIZES[r]])
def test_nms_random_sets(rotated, n):
    boxes, scores, groups = C.nms_set(n, rotated)
    iou = iou64_of(("rand", rotated, n), boxes, rotated)
    for thr in C.NMS_THRS[rotated]:
        assert hip_nms(boxes, scores, thr, rotated) == R.nms(boxes, scores, thr, iou=iou).tolist(), thr
        cfg = dict(type="nms_rotated" if rotated else "nms", iou_threshold=thr, split_thr=10)
        dets, keep = batched_nms(dev(boxes), dev(scores), dev(groups), cfg)
        assert keep.cpu().tolist() == R.nms(boxes, scores, thr, groups, iou=iou).tolist(), thr
        assert dets.shape == (keep.numel(), boxes.shape[1] + 1) and torch.equal(dets[:, -1].cpu(), torch.from_numpy(scores)[keep.cpu()])
        _, keep = batched_nms(dev(boxes), dev(scores), dev(groups), cfg, class_agnostic=True)
        assert keep.cpu().tolist() == R.nms(boxes, scores, thr, iou=iou).tolist(), thr
    if rotated:
        assert hip_nms(boxes, scores, 0.1, True, groups) == R.nms(boxes, scores, 0.1, groups, iou=iou).tolist()


@pytest.mark.parametrize("n", [C.CHAIN_N, C.CHAIN_N_WIDE])      # 33 mask words per row; 67: the scan's lanes stride twice over the column blocks
@pytest.mark.parametrize("rotated", [False, True])
def test_nms_chain_set(rotated, n):
    boxes, scores = C.chain_set(rotated, n)
    iou = iou64_of(("chain", rotated, n), boxes, rotated)
    kept = set()
    for thr in C.NMS_THRS[rotated]:
        want = R.nms(boxes, scores, thr, iou=iou).tolist()
        assert hip_nms(boxes, scores, thr, rotated) == want, thr
        kept.add(len(want))
    assert len(kept) >= 3 and min(kept) > n // C.CHAIN_LEN + 1      # chains: more than one survivor per row, and the thresholds tell apart


@pytest.mark.parametrize("rotated", [False, True])
def test_nms_identical_disjoint_and_groups(rotated):
    n = 130
    one = C.f32([[20, 30, 16, 12, 0.4]] if rotated else [[12, 24, 28, 36]])
    same = np.repeat(one, n, 0)
    scores = C.f32(np.random.default_rng(3).permutation(n) / n)
    top = int(scores.argmax())
    assert hip_nms(same, scores, 0.5, rotated) == [top]
    apart = same.copy()
    apart[:, 0] += 40 * np.arange(n, dtype=np.float32)
    if not rotated:
        apart[:, 2] += 40 * np.arange(n, dtype=np.float32)
    order = np.argsort(-scores, kind="stable").tolist()
    assert hip_nms(apart, scores, 0.5, rotated) == order
    ids = np.arange(n, dtype=np.int64) * 1000003           # identical boxes under different ids: nothing suppresses
    cfg = dict(type="nms_rotated" if rotated else "nms", iou_threshold=0.5)
    assert batched_nms(dev(same), dev(scores), dev(ids), cfg)[1].cpu().tolist() == order
    assert batched_nms(dev(same), dev(scores), dev(ids % 2), cfg)[1].cpu().tolist() == [i for i in order if i in (order[0], next(j for j in order if j % 2 != order[0] % 2))]


def test_nms_max_num_score_threshold_and_tie():
    boxes, scores, groups = C.nms_set(129, False)
    iou = iou64_of(("rand", False, 129), boxes, False)
    want = R.nms(boxes, scores, 0.5, iou=iou).tolist()
    assert len(want) > 7 and hip_nms(boxes, scores, 0.5, False, max_num=7) == want[:7]
    assert batched_nms(dev(boxes), dev(scores), dev(groups), dict(type="nms", iou_threshold=0.5, max_num=5), class_agnostic=True)[1].cpu().tolist() == want[:5]
    st = 0.5
    sel = np.nonzero(scores > st)[0]
    assert 0 < len(sel) < 129
    assert hip_nms(boxes, scores, 0.5, False, score_threshold=st) == sel[R.nms(boxes[sel], scores[sel], 0.5)].tolist()
    # the constructed tie: equal scores, the lower index first -- and it is the one that survives where the two overlap
    b = C.f32([[0, 0, 10, 10], [100, 100, 110, 110], [1, 0, 11, 10], [100, 101, 110, 111], [200, 0, 210, 10]])
    s = C.f32([0.5, 0.9, 0.5, 0.9, 0.5])
    assert hip_nms(b, s, 0.5, False) == [1, 0, 4] == R.nms(b, s, 0.5).tolist()
    assert hip_nms(b, s, 0.9, False) == [1, 3, 0, 2, 4]
    r = C.f32(C.hbox_to_rbox(b, np.zeros(5)))
    assert hip_nms(r, s, 0.5, True) == [1, 0, 4] and hip_nms(r, s, 0.9, True) == [1, 3, 0, 2, 4]


def test_nms_two_calls_give_the_same_bits():
    for rotated in (False, True):
        boxes, scores = C.chain_set(rotated)
        b, s = dev(boxes), dev(scores)
        f = nms_rotated if rotated else nms
        a, c = f(b, s, 0.5), f(b, s, 0.5)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and a[1].numel() > 100
        o = [box_iou_rotated(b[:300], b[:257]) if rotated else bbox_overlaps(b[:300], b[:257]) for _ in range(2)]
        assert torch.equal(o[0], o[1])


# ------------------------------------------------------------------------------------------------------------------- assignment
class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


CALCULATOR = {"box": "BboxOverlaps2D", "rbox2hbox": "MTP_RD_RBbox2HBboxOverlaps2D", "rotated": "RBboxOverlaps2D"}


def hip_assign(gts, priors, labels, kind, cfg, cls="MTP_RD_MaxIoUAssigner"):
    a = TASK_UTILS.build(dict(type=cls, iou_calculator=dict(type=CALCULATOR[kind]), **cfg))
    res = a.assign(Bag(priors=dev(priors)), Bag(bboxes=dev(gts), labels=dev(labels)))
    assert res.num_gts == len(gts) and res.gt_inds.dtype == I64 and res.labels.dtype == I64 and res.max_overlaps.dtype == torch.float32
    return res.gt_inds.cpu().numpy(), res.max_overlaps.cpu().numpy(), res.labels.cpu().numpy()


def check_assign(got, want, mx32, tag):
    err, e32 = err_of(got[1], want[1]), err_of(mx32, want[1])
    record_parity("box_ops", "assign_max_overlaps_" + tag, err)
    record_parity("box_ops", "assign_box_ref_f32_cpu_" + tag, e32)
    assert np.array_equal(got[0], want[0]), (tag, np.nonzero(got[0] != want[0])[0][:10])
    assert np.array_equal(got[2], want[2]), tag
    assert err < max(4 * e32, 1e-6), (tag, err, e32)


def test_assign_fixture_cases(golden):
    g = golden("f21_box_ops.npz")
    from make_box_ops import RUNS
    for cfg, kind in RUNS:
        gts, priors, labels = g[kind + ".gts"], g[kind + ".priors"], g[kind + ".labels"]
        p = "%s.%s." % (cfg, kind)
        want = (g[p + "gt_inds"], g[p + "max_overlaps"], g[p + "labels"])
        got = hip_assign(gts, priors, labels, kind, C.ASSIGN_CFGS[cfg])
        check_assign(got, want, R.overlaps(gts, priors, kind, R.F32).max(0), "f21_%s_%s" % (cfg, kind))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("K,N", C.ASSIGN_SIZES)
def test_assign_vs_float64(K, N, kind):
    gts, priors, labels, ov = C.assign_set(K, N, kind)
    mx32 = R.overlaps(gts, priors, kind, R.F32).max(0)
    seen = set()
    for name, cfg in C.ASSIGN_CFGS.items():
        want = R.assign_wrt_overlaps(ov, labels, **cfg)
        got = hip_assign(gts, priors, labels, kind, cfg, "MaxIoUAssigner" if name == "rcnn_on" else "MTP_RD_MaxIoUAssigner")
        check_assign(got, want, mx32, "%s_%dx%d_%s" % (kind, K, N, name))
        seen |= set(np.unique(np.minimum(want[0], 1)).tolist())
    if N >= 64:
        assert seen == {-1, 0, 1}


@pytest.mark.parametrize("kind", R.KINDS)
def test_assign_more_gts_than_one_tile(kind):
    """K = 300: the kernels tile the gts through LDS 256 at a time.  Gts 255 and 256 are exact duplicates across the tile boundary (the positive takes the
    lower index, low-quality matching then hands it to the higher one, in the next tile); every second gt, in both tiles, has only a prior between
    0.3 and 0.5, which the low-quality rule alone can match."""
    gts, priors, labels, ov = C.big_set(kind)
    T = C.TILE
    assert len(gts) == C.BIG_K > T and np.array_equal(gts[T - 1], gts[T]) and int(ov.argmax(0)[T - 1]) == T - 1 and ov[T, T - 1] > 0.99
    lowq = np.nonzero(ov.max(1) < 0.5)[0]
    assert (lowq < T).sum() > 50 and (lowq > T).sum() > 10 and float(ov.max(1)[lowq].min()) > 0.3
    mx32 = R.overlaps(gts, priors, kind, R.F32).max(0)
    for name, cfg in C.ASSIGN_CFGS.items():
        want = R.assign_wrt_overlaps(ov, labels, **cfg)
        got = hip_assign(gts, priors, labels, kind, cfg)
        check_assign(got, want, mx32, "%s_%dx%d_%s" % (kind, C.BIG_K, C.BIG_N, name))
        assert got[0][T - 1] == (T + 1 if cfg["match_low_quality"] else T), name
        if cfg["match_low_quality"] and cfg["min_pos_iou"] < 0.31:      # every gt is matched, the second tile's included; without the rule (or below min_pos_iou) the low ones are not
            assert set(range(1, C.BIG_K + 1)) <= set(got[0].tolist()), name
        else:
            assert not set((lowq + 1).tolist()) & set(got[0].tolist()), name
    g, p, l = dev(gts), dev(priors), dev(labels)
    r = [ops.max_iou_assign(g, p, l, kind, 0.7, 0.3, 0.3, True, True) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*r))


@pytest.mark.parametrize("kind", ["box", "rotated"])
def test_assign_duplicate_gts_and_duplicate_priors(kind):
    rot = kind == "rotated"
    g0 = [50, 60, 40, 20, 0.3] if rot else [30, 50, 70, 70]
    far = [200, 200, 30, 30, 0.0] if rot else [185, 185, 215, 215]
    shift = lambda b, d: [b[0] + d, b[1], b[2] + (0 if rot else d), b[3]] + b[4:]      # noqa: E731
    d1 = 14 if rot else 18            # an overlap between min_pos_iou = 0.3 and 0.5
    # duplicate gts 0 and 1: prior 0 (= the gt, overlap 1) is positive for the LOWER index; with low-quality matching the higher index overwrites
    gts, labels = C.f32([g0, g0, far]), np.array([3, 5, 7])
    priors = C.f32([g0, shift(g0, d1), far, shift(far, 100)])
    ov = R.overlaps(gts, priors, kind)
    assert ov[0, 0] > 0.99 and 0.3 < ov[0, 1] < 0.5 and np.array_equal(ov[0], ov[1])
    off, on = C.ASSIGN_CFGS["rcnn_off"], C.ASSIGN_CFGS["rpn"]
    got = hip_assign(gts, priors, labels, kind, off)
    assert got[0].tolist() == [1, 0, 3, 0] and got[2].tolist() == [3, -1, 7, -1] and got[0].tolist() == R.assign_wrt_overlaps(ov, labels, **off)[0].tolist()
    got = hip_assign(gts, priors, labels, kind, on)
    assert got[0].tolist() == [2, -1, 3, 0] and got[2].tolist() == [5, -1, 7, -1] and got[0].tolist() == R.assign_wrt_overlaps(ov, labels, **on)[0].tolist()
    # duplicate priors 0 and 1 at the gt's maximum (between min_pos_iou and pos_iou_thr: only the low-quality rule can match them)
    gts, labels = C.f32([g0, far]), np.array([3, 7])
    priors = C.f32([shift(g0, d1), shift(g0, d1), shift(g0, 30), far])
    ov = R.overlaps(gts, priors, kind)
    assert 0.3 < ov[0, 0] < 0.5 and ov[0, 0] == ov[0, 1] > ov[0, 2]
    for name, want in (("rpn", [1, 1, 0, 2]), ("first_only", [1, -1, 0, 2])):
        got = hip_assign(gts, priors, labels, kind, C.ASSIGN_CFGS[name])
        assert got[0].tolist() == want == R.assign_wrt_overlaps(ov, labels, **C.ASSIGN_CFGS[name])[0].tolist(), name
        assert got[2].tolist() == [3 if w == 1 else 7 if w == 2 else -1 for w in want]


@pytest.mark.parametrize("kind", ["box", "rotated"])
def test_assign_gt_that_overlaps_no_prior_at_min_pos_iou_zero(kind):
    """the reference's rule at min_pos_iou = 0 (the constructor's default): a gt whose maximum is 0 takes every prior that overlaps it by 0
    (gt_max_assign_all), or prior 0 (its first arg-max); the later gts overwrite"""
    rot = kind == "rotated"
    g0, lone = ([50, 60, 40, 20, 0.3], [900, 900, 30, 30, 0.5]) if rot else ([30, 50, 70, 70], [885, 885, 915, 915])
    far = [200, 200, 30, 30, 0.0] if rot else [185, 185, 215, 215]
    gts, labels = C.f32([lone, g0]), np.array([3, 7])
    priors = C.f32([far, g0, far, [b + (0 if i == 4 else 1) for i, b in enumerate(g0)]])
    ov = R.overlaps(gts, priors, kind)
    assert float(ov[0].max()) == 0.0 and ov[1, 1] > 0.99 > ov[1, 3] > 0.7 and ov[1, 0] == 0.0
    for all_, want in ((True, [1, 2, 1, 1]), (False, [1, 2, 0, 2])):
        cfg = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.0, match_low_quality=True, gt_max_assign_all=all_)
        got = hip_assign(gts, priors, labels, kind, cfg)
        assert got[0].tolist() == want == R.assign_wrt_overlaps(ov, labels, **cfg)[0].tolist(), all_
        assert got[2].tolist() == [3 if w == 1 else 7 if w == 2 else -1 for w in want]


@pytest.mark.parametrize("kind", R.KINDS)
def test_assign_no_gts_and_no_priors(kind):
    gts, priors, labels, _ = C.assign_set(3, 65, kind)
    a = MaxIoUAssigner(0.7, 0.3, iou_calculator=dict(type="mmdet." + CALCULATOR[kind]))
    res = a.assign(Bag(priors=dev(priors)), Bag(bboxes=dev(gts[:0]), labels=dev(labels[:0])))
    assert res.num_gts == 0 and res.gt_inds.is_cuda and res.gt_inds.cpu().tolist() == [0] * 65 and res.labels.cpu().tolist() == [-1] * 65
    assert res.max_overlaps.dtype == torch.float32 and float(res.max_overlaps.abs().max()) == 0.0
    res = a.assign(Bag(priors=dev(priors[:0])), Bag(bboxes=dev(gts), labels=dev(labels)))
    assert res.num_gts == 3 and res.gt_inds.shape == res.labels.shape == res.max_overlaps.shape == (0,) and res.gt_inds.is_cuda


def test_assign_two_calls_give_the_same_bits():
    for kind in R.KINDS:
        gts, priors, labels, _ = C.assign_set(65, 1000, kind)
        g, p, l = dev(gts), dev(priors), dev(labels)
        r = [ops.max_iou_assign(g, p, l, kind, 0.7, 0.3, 0.3, True, True) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(*r))
