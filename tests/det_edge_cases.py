"""Input sets of the detection-head edge tests (tests/test_hip_det_edges.py) and the conditions they must meet, from the float64 references (roi_ref,
rpn_ref, box_ref) alone.  Plain helper module: no tests, no fixtures.  tests/test_det_edges_host.py asserts every condition on the CPU.
Two kinds of case:
  * exact: dyadic inputs for which the float32 and the float64 run of the reference coincide (the float64 result, cast to float32, IS the float32
    result), so the GPU test compares with torch.equal;
  * close: random inputs, seed-rejected under the gaps of roi_cases / rpn_cases, compared with `held`: the kernel's error against float64 below
    4 x the error of the float32 CPU restatement against float64, floor 1e-6.  No RoI, row or element is masked out of a comparison.
The seeds are the first that pass (python tests/det_edge_cases.py prints them)."""
import functools

import numpy as np

import box_cases as BC
import roi_cases as RC
import roi_ref as R
import rpn_cases as PC
import rpn_ref as PR
from conftest import record_parity

F64, F32 = np.float64, np.float32
CUT_GAP, LEVEL_GAP, ANGLE_GAP, SHAPE_GAP, SCORE_GAP = RC.CUT_GAP, RC.LEVEL_GAP, RC.ANGLE_GAP, RC.SHAPE_GAP, RC.SCORE_GAP
STRIDES, FINEST, BATCH = RC.STRIDES, RC.FINEST, RC.BATCH
MEANS, STDS = RC.MEANS, RC.STDS


def err_of(a, ref):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return float(np.abs(a.astype(F64) - ref).max()) if ref.size else 0.0


def held(tag, out, ref64, ref32):
    """the rule of tests/test_hip_roi.py: 4 x the float32 CPU error of the restatement against float64, floor 1e-6; both numbers recorded"""
    ref64 = np.asarray(ref64, F64)
    err, e32 = err_of(out, ref64), err_of(ref32, ref64)
    record_parity("det_edges", tag, err)
    record_parity("det_edges", "ref_f32_cpu_" + tag, e32)
    print("%s: err %.3e, float32 restatement %.3e" % (tag, err, e32))
    assert tuple(out.shape) == ref64.shape and err < max(4 * e32, 1e-6), (tag, err, e32)


def same32(a64, a32):
    """an exact case: the float64 run, cast to float32, is the float32 run bit for bit"""
    a64, a32 = np.asarray(a64), np.asarray(a32)
    return a32.dtype == F32 and a64.dtype == F64 and a64.shape == a32.shape and np.array_equal(a64.astype(F32).view(np.uint32), a32.view(np.uint32))


def bin_major(x):
    """(R, C, P, P) -> the kernels' (R, P P, C)"""
    return np.ascontiguousarray(np.transpose(x.reshape(x.shape[0], x.shape[1], -1), (0, 2, 1)))


def rows_of(maps, ld):
    """NCHW maps -> per level (N H W, ld) rows whose first C columns are the channels"""
    out = []
    for m in maps:
        N, Cc, H, W = m.shape
        r = np.zeros((N * H * W, ld), F32)
        r[:, :Cc] = np.transpose(m, (0, 2, 3, 1)).reshape(-1, Cc)
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------------------------- RoIAlignRotated: reference helpers
def roi_align_bwd(dout, shapes, rois, strides, P, S, clockwise, finest_scale=FINEST, levels=None, valid=None, dtype=F64):
    """roi_ref.roi_align_bwd with the additions into the pixels made by np.add.at per RoI: the same products added in the same order (bin, sample,
    corner), so the same bits in either precision (tests/test_det_edges_host.py holds the two equal); the edge cases have up to 1024 points a RoI"""
    dout = np.asarray(dout, dtype)
    rois = np.asarray(rois, dtype).reshape(-1, 6)
    levels = R.map_levels(rois, len(shapes), finest_scale, dtype) if levels is None else np.asarray(levels)
    grads = [np.zeros(s, dtype) for s in shapes]
    count = dtype(max(S * S, 1))
    Rn, C = dout.shape[:2]
    d = dout.reshape(Rn, C, P * P)
    for r in range(Rn):
        if valid is not None and not valid[r]:
            continue
        g = grads[levels[r]]
        H, W = g.shape[2:]
        y, x = R.sample_points(rois[r], H, W, 1.0 / strides[levels[r]], P, S, clockwise, dtype)
        inside, (yl, yh, xl, xh), w = R.bilinear(y, x, H, W, dtype)
        ys, xs = np.stack([yl, yl, yh, yh], 2), np.stack([xl, xh, xl, xh], 2)      # (P P, S S, 4): the loop order of roi_ref
        ws = (np.stack(w, 2) / count).astype(dtype)
        keep = np.broadcast_to(inside[:, :, None], ys.shape).reshape(-1)
        bins = np.broadcast_to(np.arange(P * P)[:, None, None], ys.shape).reshape(-1)[keep]
        vals = (ws.reshape(-1)[keep][None, :] * d[r][:, bins]).astype(dtype)
        np.add.at(g[int(rois[r, 0])], (slice(None), ys.reshape(-1)[keep], xs.reshape(-1)[keep]), vals)
    return grads


def roi_align_cut(maps, rois, strides, P, S, clockwise, levels, lo_open=False, hi_open=False, dtype=F64):
    """roi_ref.roi_align from roi_ref's own sample_points and bilinear, with the cut-off comparisons optionally made exclusive: lo_open counts a
    sample at exactly -1 outside, hi_open one at exactly H or W.  With both closed it is roi_align (held equal in the host test); an exact cut-off
    case must change under either flag, or it would not tell `>=` from `>`."""
    maps = [np.asarray(m, dtype) for m in maps]
    rois = np.asarray(rois, dtype).reshape(-1, 6)
    out = np.zeros((len(rois), maps[0].shape[1], P * P), dtype)
    for r in range(len(rois)):
        m = maps[levels[r]]
        H, W = m.shape[2:]
        y, x = R.sample_points(rois[r], H, W, 1.0 / strides[levels[r]], P, S, clockwise, dtype)
        inside, (yl, yh, xl, xh), w = R.bilinear(y, x, H, W, dtype)
        if lo_open:
            inside = inside & (y != -1) & (x != -1)
        if hi_open:
            inside = inside & (y != H) & (x != W)
        f = m[int(rois[r, 0])]
        acc = np.zeros((maps[0].shape[1], P * P), dtype)
        for s in range(S * S):
            val = ((w[0][:, s] * f[:, yl[:, s], xl[:, s]] + w[1][:, s] * f[:, yl[:, s], xh[:, s]]) + w[2][:, s] * f[:, yh[:, s], xl[:, s]]) \
                + w[3][:, s] * f[:, yh[:, s], xh[:, s]]
            acc = acc + np.where(inside[:, s], val, dtype(0))
        out[r] = acc / dtype(max(S * S, 1))
    return out.reshape(len(rois), -1, P, P)


def margins_ok(rois, levels, sizes, strides, P, S, clockwise, computed=True):
    """CUT_GAP on every sample coordinate and, where the level is computed from the RoI, LEVEL_GAP on the level map"""
    if computed and not (R.level_margin(rois, FINEST) > LEVEL_GAP).all():
        return False
    return bool(R.cutoff_margin(rois, levels, sizes, strides, P, S, clockwise) > CUT_GAP)


# ------------------------------------------------------------------------------------------------------------------- 1a. wide channels
WIDE_C = (64, 65, 130)      # gridDim.y of roi_align_gather_kernel: 1, 2 with one live lane in the second block, 3


@functools.lru_cache(maxsize=None)
def wide_case(channels):
    """the RoIs of roi_cases.align_case (24, built by roi_cases._align_try: its conditions hold, tests/test_roi_host.py) on maps of `channels`"""
    rois = RC.align_case()[1]
    rng = np.random.default_rng(2400 + channels)
    return [BC.f32(rng.normal(0.0, 1.0, (BATCH, channels, H, W))) for H, W in RC.sizes_of((128, 128))], rois


# ------------------------------------------------------------------------------------------------------------------- 1b. geometry sweep
# (out_size, sample_num, clockwise); the last three sit on the limit of 1024 points
GEOMS = ((1, 1, True), (7, 1, True), (7, 3, True), (7, 3, False), (3, 2, True), (3, 2, False), (14, 2, True), (8, 4, False), (16, 2, True), (32, 1, False))
GEOM_REFUSED = ((8, 5), (33, 1))
GEOM_C = 8


def _geom_try(seed):
    """12 RoIs in the manner of roi_cases._align_try: the four levels and both clamped ends, partly and wholly outside, sub-pixel, theta near 0, +-pi/2"""
    rng = np.random.default_rng(2500 + seed)
    j = lambda: rng.uniform(-3, 3)      # noqa: E731
    rois = [
        [0, 40 + j(), 50 + j(), 30, 18, 0.3], [1, 64 + j(), 60 + j(), 190, 120, -0.7], [0, 70 + j(), 64 + j(), 330, 300, 1.1],
        [1, 60 + j(), 66 + j(), 520, 470, -0.2], [0, 64 + j(), 64 + j(), 2100, 1900, 0.5], [1, 30 + j(), 90 + j(), 5, 3, -1.0],
        [0, 6 + j(), 120 + j(), 40, 22, 0.8], [1, -400 + j(), -300 + j(), 20, 12, 0.4], [0, 77.3 + j(), 41.6 + j(), 0.6, 0.4, 0.2],
        [1, 50 + j(), 70 + j(), 44, 20, 0.004], [0, 80 + j(), 44 + j(), 36, 24, np.pi / 2 - 0.004], [1, 44 + j(), 84 + j(), 52, 16, -np.pi / 2 + 0.004]]
    return BC.f32(np.asarray(rois))


def geom_condition(rois, P, S, clockwise):
    lv = R.map_levels(rois, len(STRIDES), FINEST)
    return set(lv.tolist()) == {0, 1, 2, 3} and margins_ok(rois, lv, RC.sizes_of((128, 128)), STRIDES, P, S, clockwise)


GEOM_SEEDS = {}      # filled below: (P, S, clockwise) -> seed


@functools.lru_cache(maxsize=None)
def geom_maps():
    rng = np.random.default_rng(2499)
    return [BC.f32(rng.normal(0.0, 1.0, (BATCH, GEOM_C, H, W))) for H, W in RC.sizes_of((128, 128))]


@functools.lru_cache(maxsize=None)
def geom_case(P, S, clockwise):
    return geom_maps(), _geom_try(GEOM_SEEDS[(P, S, clockwise)])


# ------------------------------------------------------------------------------------------------------------------- 1c. exact cut-offs
EXACT_P, EXACT_S, EXACT_STRIDE, EXACT_HW, EXACT_C = 4, 2, 4, 8, 3
# (image, cx, cy, w, h, 0) at scale 1/4 on an 8 x 8 map: bins of 2 pixels, samples one pixel apart, on
EXACT_ROIS = np.array([
    [0, 12, 12, 32, 32, 0],      # x, y = -1, 0, ..., 6: the low cut-off on both axes, integer pixels (zero high weights)
    [1, 20, 20, 32, 32, 0],      # x, y = 1, ..., 8: H - 1 = 7 (the clamp branch) and the high cut-off H = W = 8
    [0, 20, 12, 32, 32, 0],      # y = -1, ..., 6 with x = 1, ..., 8: the -1 row with the W column
    [1, 12, 20, 32, 32, 0],      # and the H row with the -1 column
    [0, 14, 18, 32, 32, 0],      # x = -0.5, ..., 6.5 and y = 0.5, ..., 7.5: half weights, the clamp of negatives to 0 and of 7.5 to 7
], F32)


@functools.lru_cache(maxsize=None)
def exact_case():
    """(maps [(2, C, 8, 8)] integer-valued, rois, dout (R, C, 4, 4) in quarters)"""
    rng = np.random.default_rng(2600)
    m = rng.integers(-8, 9, (2, EXACT_C, EXACT_HW, EXACT_HW)).astype(F32)
    dout = (rng.integers(-8, 9, (len(EXACT_ROIS), EXACT_C, EXACT_P, EXACT_P)) / 4.0).astype(F32)
    return [m], EXACT_ROIS, dout


def exact_samples(roi, clockwise):
    return R.sample_points(roi, EXACT_HW, EXACT_HW, 1.0 / EXACT_STRIDE, EXACT_P, EXACT_S, clockwise)


# ------------------------------------------------------------------------------------------------------------------- 1d. one-pixel maps
PIXEL_SIZES, PIXEL_STRIDES, PIXEL_C, PIXEL_P, PIXEL_S = ((1, 1), (1, 5), (5, 1)), (4, 4, 4), 4, 7, 2


def _pixel_try(seed):
    """per level four RoIs (roi_levels overrides the level map): inside the map, about its size, hanging over it, turned"""
    rng = np.random.default_rng(2700 + seed)
    rois, lv = [], []
    for l, (H, W) in enumerate(PIXEL_SIZES):
        cx, cy = 2.0 * W, 2.0 * H      # the centre of the map in image coordinates
        for k, (fw, fh, th) in enumerate(((0.4, 0.4, 0.3), (1.0, 1.0, -0.2), (4.0, 4.0, 0.9), (1.5, 0.7, np.pi / 2 - 0.1))):
            rois.append([k % BATCH, cx + rng.uniform(-1.5, 1.5), cy + rng.uniform(-1.5, 1.5), 4 * W * fw * rng.uniform(0.8, 1.2), 4 * H * fh * rng.uniform(0.8, 1.2), th])
            lv.append(l)
    return BC.f32(np.asarray(rois)), np.asarray(lv, np.int64)


def pixel_condition(case):
    rois, lv = case
    if not margins_ok(rois, lv, PIXEL_SIZES, PIXEL_STRIDES, PIXEL_P, PIXEL_S, True, computed=False):
        return False
    out = R.roi_align(pixel_maps(), rois, PIXEL_STRIDES, PIXEL_P, PIXEL_S, True, FINEST, levels=lv)
    zero = (out == 0).all(1).reshape(len(rois), -1)      # bins wholly outside
    return bool((~zero).any(1).all() and zero[2::4].any(1).all())      # every RoI reads its map; the one that hangs over has bins outside it


@functools.lru_cache(maxsize=None)
def pixel_maps():
    rng = np.random.default_rng(2699)
    return [BC.f32(rng.normal(0.0, 1.0, (BATCH, PIXEL_C, H, W))) for H, W in PIXEL_SIZES]


PIXEL_SEED = 1


@functools.lru_cache(maxsize=None)
def pixel_case():
    return _pixel_try(PIXEL_SEED)


# ------------------------------------------------------------------------------------------------------------------- 1e. slots that are not RoIs
NAN = float("nan")
# four RoIs proper, then (image, cx, cy, w, h, theta) whose image index names no image, then a valid image with sizes that are NaN, zero, negative
SLOT_ROIS = np.array([
    [0, 41.3, 50.2, 30, 18, 0.3], [1, 64.4, 60.9, 190, 120, -0.7], [0, 70.1, 64.7, 330, 300, 1.1], [1, 60.6, 66.2, 520, 470, -0.2],
    [-1, 40, 50, 30, 18, 0.3], [BATCH, 40, 50, 30, 18, 0.3], [BATCH + 0.5, 40, 50, 30, 18, 0.3], [NAN, 40, 50, 30, 18, 0.3],
    [0, 40, 50, NAN, 18, 0.3], [1, 40, 50, 30, NAN, 0.3],
    [0, 41.7, 50.9, 0, 18, 0.3], [1, 43.1, 52.3, 30, 0, 0.3], [0, 45.9, 49.3, -30, 18, 0.3], [1, 47.3, 53.1, -30, -18, 0.3]], F32)
SLOT_BAD_IMAGE, SLOT_NAN_SIZE, SLOT_FINITE = slice(4, 8), slice(8, 10), [0, 1, 2, 3, 10, 11, 12, 13]
# the level of every slot, stated directly (roi_level of roi_head.hip: floor(log2(sqrt(w h) / 56 + 1e-6)), below 1 or NaN -> 0, clamped to the
# last level): w h = 540, 22800, 99000, 244400 -> levels 0, 1, 2, 3; a NaN or zero or negative product -> 0; (-30)(-18) = 540 -> 0
SLOT_LEVELS = np.array([0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.int64)
SLOT_LEVELS_OUT = np.array([0, 1, 2, 3, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0], np.int64)      # levels_out: -1 where the slot is not in use
SLOT_OVERRIDE = np.array([-3, 99, -3, 99], np.int32)      # on the four RoIs proper: clamped to the first and the last level


def slot_valid():
    """what the reference is asked to compute: the slots whose image index is an image and whose sizes are numbers"""
    v = np.zeros(len(SLOT_ROIS), bool)
    v[SLOT_FINITE] = True
    return v


def slot_rois_for_ref():
    """the RoIs with the slots that are not in use made harmless for numpy (the reference skips them through `valid`)"""
    r = SLOT_ROIS.copy()
    r[~slot_valid()] = SLOT_ROIS[0]
    return r


# ------------------------------------------------------------------------------------------------------------------- 1f. hot pixel
HOT_COPIES, HOT_C = 48, 4
# both smaller than a pixel of level 0 (stride 4); the first lies in pixels x 10..11, y 7..8, the second in x 11..12, y 7..8: they share two
HOT_ROIS = np.array([[0, 44.1, 32.3, 1.6, 1.2, 0.2], [0, 48.3, 32.1, 1.2, 1.6, -0.3]], F32)


@functools.lru_cache(maxsize=None)
def hot_case():
    rois = np.repeat(HOT_ROIS, HOT_COPIES, 0)
    rng = np.random.default_rng(2800)
    dout = rng.normal(0, 1, (len(rois), HOT_C, RC.P, RC.P)).astype(F32)
    return rois, dout


# ------------------------------------------------------------------------------------------------------------------- 1g. smallest
SMALL_ROI, SMALL_STRIDE = np.array([[0, 9.3, 11.1, 10, 7, 0.4]], F32), 4


@functools.lru_cache(maxsize=None)
def small_case():
    """R = 1, one level, N = 1, C = 1: (maps [(1, 1, 6, 5)], rois, dout (1, 1, 7, 7))"""
    rng = np.random.default_rng(2850)
    return [BC.f32(rng.normal(0, 1, (1, 1, 6, 5)))], SMALL_ROI, BC.f32(rng.normal(0, 1, (1, 1, RC.P, RC.P)))


# ------------------------------------------------------------------------------------------------------------------- 2a. RoI loss: chunk seams
BETA = 1.0
# (S, images, K, pad): every S and every K of the issue at least once; roi_loss_kernel has a second chunk from S = 257 on
LOSS_CASES = ((1, 1, 1, 0), (255, 3, 5, 3), (256, 1, 15, 0), (257, 3, 80, 3), (512, 2, 15, 3), (600, 1, 80, 0), (600, 3, 5, 3))
NUM_G = 7


def loss_counts(S, images):
    """per image (n_pos, n_neg): full, partial with its last slot in the last chunk, zero; n_pos = 0 on the partial one when there are two images"""
    full, part, zero = (S // 4, S - S // 4), (min(3, S - 1), max(S - 5, 0) if S > 4 else 0), (0, 0)
    if images == 1:
        return [part if S > 1 else (1, 0)]
    if images == 2:
        return [full, (0, S - 2)]
    return [full, part, zero]


def _loss_try(S, images, K, seed):
    """dict: cls (B S, K + 1), reg (B S, 5), rois (B S, 5), gts (G, 5), gt_labels, sample_gt (B, S), n_pos, n_neg"""
    rng = np.random.default_rng(2900 + 7 * S + images + 1000 * seed)
    n = images * S
    gts = np.stack([rng.uniform(20, 108, NUM_G), rng.uniform(20, 108, NUM_G), rng.uniform(14, 90, NUM_G), rng.uniform(8, 60, NUM_G),
                    rng.uniform(-np.pi / 2 + 0.05, np.pi / 2 - 0.05, NUM_G)], 1)
    sg = rng.integers(0, NUM_G, (images, S))
    rois = gts[sg.reshape(-1)].copy()      # every slot a jittered copy of its gt; a third of them turned by about a quarter turn
    rois[:, :2] += rng.uniform(-2, 2, (n, 2))
    rois[:, 2:4] *= rng.uniform(0.85, 1.15, (n, 2))
    rois[:, 4] += rng.uniform(-0.1, 0.1, n)
    turn = rng.uniform(0, 1, n) < 0.33
    rois[turn] = np.stack([rois[turn, 0], rois[turn, 1], rois[turn, 3], rois[turn, 2], rois[turn, 4] + np.pi / 2 * np.where(rois[turn, 4] < 0, 1, -1)], 1)
    counts = loss_counts(S, images)
    return dict(cls=BC.f32(rng.normal(0, 1.5, (n, K + 1))), reg=BC.f32(rng.normal(0, 1.0, (n, 5))), rois=BC.f32(rois), gts=BC.f32(gts),
                gt_labels=rng.integers(0, K, NUM_G).astype(np.int64), sample_gt=sg.astype(np.int64), n_pos=np.array([c[0] for c in counts], np.int64),
                n_neg=np.array([c[1] for c in counts], np.int64), K=K, S=S, images=images)


def loss_condition(c):
    """encode: the positives clear of the d1 / d2 choice and of the wrap; acc: the top-1 margin of every slot in use above SCORE_GAP"""
    S = c["S"]
    used = np.concatenate([b * S + np.arange(c["n_pos"][b] + c["n_neg"][b]) for b in range(c["images"])]).astype(np.int64)
    pos = np.concatenate([b * S + np.arange(c["n_pos"][b]) for b in range(c["images"])]).astype(np.int64)
    gap, wrap = R.angle_margins(c["rois"][pos], c["gts"][c["sample_gt"].reshape(-1)[pos]])
    return bool((gap > ANGLE_GAP).all() and (wrap > ANGLE_GAP).all() and R.top1_margin(c["cls"], used) > SCORE_GAP)


LOSS_SEEDS = {}      # filled below: (S, images, K) -> seed


@functools.lru_cache(maxsize=None)
def loss_case(S, images, K):
    return _loss_try(S, images, K, LOSS_SEEDS[(S, images, K)])


def loss_ref(c, dtype=F64, beta=BETA, **over):
    c = dict(c, **over)
    return R.loss(c["cls"], c["reg"], c["K"], c["rois"], c["gts"], c["gt_labels"], c["sample_gt"], c["n_pos"], c["n_neg"], MEANS, STDS, beta, dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------- 2b. device-side clamps
def clamp_counts(n_pos, n_neg, S):
    """sample_counts of roi_head.hip, written out:  np = np < 0 ? 0 : (np > S ? S : np);  nn = nn < 0 ? 0 : (nn > S - np ? S - np : nn)"""
    n_pos = np.clip(np.asarray(n_pos, np.int64), 0, S)
    return n_pos, np.minimum(np.clip(np.asarray(n_neg, np.int64), 0, None), S - n_pos)


CLAMP_S, CLAMP_K, CLAMP_SEED = 40, 5, 0


def clamp_condition(seed):
    """any slot may be a positive once the counts are clamped: loss_condition with every slot a positive"""
    c = dict(_loss_try(CLAMP_S, 4, CLAMP_K, seed))
    c["n_pos"], c["n_neg"] = np.full(4, CLAMP_S, np.int64), np.zeros(4, np.int64)
    return loss_condition(c)


@functools.lru_cache(maxsize=None)
def clamp_case():
    """four images of CLAMP_S slots from the S = 40 draw.  What the kernel is given, and what that means once cleaned:
       image 0: n_pos -4, n_neg 12                       -> 0 positives, 12 negatives
       image 1: n_pos S + 9, n_neg 3                      -> S positives, 0 negatives
       image 2: n_pos 10, n_neg S                         -> 10 positives, S - 10 negatives
       image 3: n_pos 8, n_neg 6, sample_gt of slots 6, 7 = -1, G: `pos = g >= 0 && g < G` fails, the slot counts as a negative labelled background
                with no box term                          -> 6 positives, 8 negatives
       gt labels -2 and K + 3: `if (label < 0 || label > K) label = K`: background, the box term stays"""
    c = dict(_loss_try(CLAMP_S, 4, CLAMP_K, CLAMP_SEED))
    given = dict(n_pos=np.array([-4, CLAMP_S + 9, 10, 8], np.int64), n_neg=np.array([12, 3, CLAMP_S, 6], np.int64), sample_gt=c["sample_gt"].copy(),
                 gt_labels=c["gt_labels"].copy())
    given["sample_gt"][3, 6], given["sample_gt"][3, 7] = -1, NUM_G
    given["gt_labels"][1], given["gt_labels"][4] = -2, CLAMP_K + 3
    n_pos, n_neg = clamp_counts(given["n_pos"], given["n_neg"], CLAMP_S)
    assert n_pos.tolist() == [0, CLAMP_S, 10, 8] and n_neg.tolist() == [12, 0, CLAMP_S - 10, 6]
    n_pos[3], n_neg[3] = 6, 8      # the two slots whose gt index names no gt are the last two positives: negatives
    labels = np.where((given["gt_labels"] < 0) | (given["gt_labels"] > CLAMP_K), CLAMP_K, given["gt_labels"])
    clean = dict(n_pos=n_pos, n_neg=n_neg, sample_gt=c["sample_gt"], gt_labels=labels)
    return c, given, clean


# ------------------------------------------------------------------------------------------------------------------- 2c. softmax regimes
def softmax_rows(K, z, labels_right):
    """four slots, two positives then two negatives, rois = gts at theta 0 and zero deltas (no box loss): logits z (4, K + 1)"""
    gts = np.array([[40, 40, 32, 16, 0], [80, 72, 24, 12, 0]], F32)
    return dict(cls=BC.f32(z), reg=np.zeros((4, 5), F32), rois=gts[[0, 1, 0, 1]], gts=gts, gt_labels=np.asarray(labels_right, np.int64),
                sample_gt=np.array([[0, 1, -1, -1]], np.int64), n_pos=np.array([2], np.int64), n_neg=np.array([2], np.int64), K=K, S=4, images=1)


def softmax_cases():
    """name -> (case, exact)"""
    K = 5
    out = {}
    out["equal_label0"] = (softmax_rows(K, np.full((4, K + 1), 3.0), [0, 0]), False)      # argmax is index 0: both positives hit, both negatives miss
    out["equal_label3"] = (softmax_rows(K, np.full((4, K + 1), 3.0), [3, 2]), False)      # nobody hits
    z = np.zeros((4, K + 1))
    z[0, 2] = z[1, 4] = z[2, K] = z[3, 1] = 200.0      # slots 0 and 2 labelled right (gt 0 has label 2; background), 1 and 3 labelled wrong
    out["ahead200"] = (softmax_rows(K, z, [2, 0]), True)
    rng = np.random.default_rng(3000)
    out["offset_-1e4"] = (softmax_rows(K, BC.f32(rng.normal(0, 1.5, (4, K + 1))) - 1e4, [1, 4]), False)
    out["K1"] = (softmax_rows(1, BC.f32(rng.normal(0, 1.5, (4, 2))), [0, 0]), False)
    return out


# ------------------------------------------------------------------------------------------------------------------- 2d. SmoothL1 kinks
KINK_BETAS = (1.0, 0.25)
KINK_FACTORS = (0.0, 1.0, -1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20)


def kink_case(beta, factor):
    """one positive slot whose prior is its gt (theta 0, zero means: every target exactly 0) and whose five deltas are all beta * factor"""
    gts = np.array([[48, 40, 32, 16, 0]], F32)
    v = F32(beta) * F32(factor)
    return dict(cls=np.zeros((1, 3), F32), reg=np.full((1, 5), v, F32), rois=gts.copy(), gts=gts, gt_labels=np.array([1], np.int64),
                sample_gt=np.array([[0]], np.int64), n_pos=np.array([1], np.int64), n_neg=np.array([0], np.int64), K=2, S=1, images=1)


def kink_expected(beta, factor):
    """(loss_bbox, dreg row) written out from the definition, in exact arithmetic rounded once to float32 per term as the kernel rounds"""
    v = F32(beta) * F32(factor)
    ad = abs(v)
    if ad < F32(beta):
        term, grad = F32(F32(F32(0.5) * ad) * ad) / F32(beta), v / F32(beta)
    else:
        term, grad = ad - F32(0.5) * F32(beta), F32(np.sign(v))
    return F32(5) * F32(term), np.full(5, grad, F32)


# ------------------------------------------------------------------------------------------------------------------- 2e. predict
PREDICT_CASES = ((1, 1, 0), (255, 15, 3), (256, 80, 0), (257, 15, 3), (1000, 80, 3), (1000, 1, 0))      # (R, K, pad): a second workgroup from R = 257 on
SCORE_THR = 0.05


def _predict_try(Rn, K, seed):
    """rows as tests/test_hip_roi.py::test_coder_decode has them: both clamps among the first six; the rows within SHAPE_GAP / ANGLE_GAP of the edge
    swap or of the wrap are replaced by the next clear ones (chosen from float64 alone, before anything runs)"""
    rng = np.random.default_rng(3100 + Rn + 7 * K + 1000 * seed)
    n = 3 * Rn + 24
    p = np.concatenate([rng.uniform(20, 100, (n, 2)), rng.uniform(8, 60, (n, 2)), rng.uniform(-np.pi / 2, np.pi / 2, (n, 1))], 1).astype(F32)
    d = rng.normal(0, 1.0, (n, 5)) * np.array([1, 1, 2, 2, 4])
    if Rn > 20:
        d[:6, 2], d[:6, 3] = [45, -45, 25, 21, -21, 0], [0, 45, -45, -25, 21, -21]
    d = d.astype(F32)
    ref, gw, gh, ga = R.decode(p, d, MEANS, STDS, swapped=True)
    fine = (np.abs(gw - gh) > SHAPE_GAP * np.maximum(gw, gh)) & (np.abs(np.abs(ga) - np.pi / 2) > ANGLE_GAP) & (np.abs(np.abs(ref[:, 4]) - np.pi / 2) > ANGLE_GAP)
    keep = np.nonzero(fine)[0][:Rn]
    return dict(rois=p[keep], reg=d[keep], cls=BC.f32(rng.normal(0, 2.0, (len(keep), K + 1))), K=K, clamped=int((keep < 6).sum()) if Rn > 20 else 0,
                swapped=(gw > gh)[keep])


def predict_condition(c, Rn):
    sc = R.softmax(c["cls"])[:, :c["K"]]
    # score_thr = 0 asks s > 0: every score is a normal float32 by a wide margin; score_thr = 1 asks s > 1: no softmax score is, in any precision
    ok = len(c["rois"]) == Rn and (np.abs(sc - SCORE_THR) > SCORE_GAP).all() and sc.min() > 1e-30
    if Rn > 20:
        ok = ok and c["clamped"] >= 4 and c["swapped"].any() and (~c["swapped"]).any()      # the clamps and both sides of the edge swap are compared
    return bool(ok)


PREDICT_SEEDS = {}


@functools.lru_cache(maxsize=None)
def predict_case(Rn, K):
    return _predict_try(Rn, K, PREDICT_SEEDS[(Rn, K)])


# ------------------------------------------------------------------------------------------------------------------- 3a. RPN loss: chunk seams
RPN_S = (255, 256, 257, 600)      # rpn_loss_kernel has a second chunk from S = 257 on
RPN_NAME = "sq128"


def rpn_counts(S):
    """per image (n_pos, n_neg): full; partial, its last slot in the last chunk"""
    return [(S // 4, S - S // 4), (5, S - 5 - 1 if S > 256 else (S - 5) // 2)]


@functools.lru_cache(maxsize=None)
def rpn_seam_case(S):
    """samples (B, S) drawn from the anchors inside the image without repeats, positives first with a gt of their image each, then negatives; the
    maps, gts and anchors are those of rpn_cases' sq128.  -> dict(samples, sample_gt (rows of the concatenated gts), n_pos, n_neg, pos, pgt, neg)"""
    cls, reg, gts = PC.case(RPN_NAME)
    priors, inside, sizes = PC.anchors(RPN_NAME)
    rng = np.random.default_rng(3200 + S)
    cand = np.nonzero(inside)[0]
    samples, sample_gt = np.zeros((BATCH, S), np.int64), -np.ones((BATCH, S), np.int64)
    pos, pgt, neg, off = [], [], [], 0
    counts = rpn_counts(S)
    for b, (np_, nn) in enumerate(counts):
        samples[b] = cand[rng.permutation(len(cand))[:S]]
        g = rng.integers(0, len(gts[b]), np_)
        sample_gt[b, :np_] = g + off
        pos.append(samples[b, :np_])
        pgt.append(g)
        neg.append(samples[b, np_:np_ + nn])
        off += len(gts[b])
    return dict(samples=samples, sample_gt=sample_gt, n_pos=np.array([c[0] for c in counts], np.int64), n_neg=np.array([c[1] for c in counts], np.int64),
                pos=pos, pgt=pgt, neg=neg)


def rpn_seam_levels(c, S):
    """per level and chunk of 256 slots, the number of samples in use: (levels, chunks)"""
    _, _, sizes = PC.anchors(RPN_NAME)
    out = np.zeros((len(sizes), -(-S // 256)), np.int64)
    for b in range(BATCH):
        used = int(c["n_pos"][b] + c["n_neg"][b])
        lv = PR.level_of(c["samples"][b, :used], sizes, PC.A)[0]
        np.add.at(out, (lv, np.arange(used) // 256), 1)
    return out


def rpn_loss_ref(c, dtype=F64, **kw):
    cls, reg, gts = PC.case(RPN_NAME)
    priors, _, sizes = PC.anchors(RPN_NAME)
    return PR.loss(cls, reg, sizes, PC.A, priors, gts, c["pos"], c["pgt"], c["neg"], PC.MEANS, PC.STDS, PC.BETA, dtype=dtype, **kw)


# ------------------------------------------------------------------------------------------------------------------- 3b. RPN loss: out-of-range entries
RPN_BAD_S = 40


@functools.lru_cache(maxsize=None)
def rpn_bad_case():
    """What rpn_loss_kernel is given, and what it means (`active = idx >= 0 && idx < total`; `if (g >= 0 && g < K)` guards the box term;
    sample_counts clamps n_pos to S and n_neg to S - n_pos; avg_factor is the sum of the clamped counts, skipped slots included):
       image 0: n_pos 6, n_neg 20; the sample indices of slots 2 and 9 are -1 and num_priors: skipped; sample_gt of slot 4 is K (the number of gts):
                a positive for the classification without a box term
       image 1: n_pos S + 7, n_neg 5 -> S positives, no negatives
    -> (given dict for the kernel, cleaned lists for rpn_ref.loss, avg_factor)"""
    S = RPN_BAD_S
    cls, reg, gts = PC.case(RPN_NAME)
    priors, inside, sizes = PC.anchors(RPN_NAME)
    K = sum(len(g) for g in gts)
    rng = np.random.default_rng(3300)
    cand = np.nonzero(inside)[0]
    samples = np.stack([cand[rng.permutation(len(cand))[:S]] for _ in range(BATCH)])
    local = np.stack([rng.integers(0, len(gts[b]), S) for b in range(BATCH)])
    sample_gt = local + np.array([[0], [len(gts[0])]])
    given = dict(samples=samples.copy(), sample_gt=sample_gt.copy(), n_pos=np.array([6, S + 7], np.int64), n_neg=np.array([20, 5], np.int64))
    given["samples"][0, 2], given["samples"][0, 9], given["sample_gt"][0, 4] = -1, len(priors), K
    pgt0 = local[0, :6].copy()
    pgt0[4] = -1
    keep_pos, keep_neg = [0, 1, 3, 4, 5], [j for j in range(6, 26) if j != 9]
    clean = dict(pos=[samples[0, keep_pos], samples[1]], pgt=[pgt0[keep_pos], local[1]], neg=[samples[0, keep_neg], samples[1, :0]])
    return given, clean, 26 + S


# ------------------------------------------------------------------------------------------------------------------- 3c. proposals
PROP_MIN_SIZE = 8.0
# name -> (A, sizes, strides, keep_counts or None for "filled in": see prop_case)
PROP_SHAPES = {"A1": (1, ((4, 4), (3, 2), (2, 2)), (8, 16, 32)), "A9": (9, ((4, 4), (3, 2), (2, 2)), (8, 16, 32)), "single": (3, ((5, 3),), (8,))}


def _prop_try(name, seed):
    """a level cut to 5, a level with keep_count 0 between levels that keep, a level kept whole; keep indices drawn without repeats"""
    A, sizes, strides = PROP_SHAPES[name]
    rng = np.random.default_rng(3400 + 1000 * seed + A)
    scales, ratios = ((8,), (1.0,)) if A == 1 else (((4, 8, 16), (0.5, 1.0, 2.0)) if A == 9 else ((8,), (0.5, 1.0, 2.0)))
    priors = np.concatenate([PR.grid_priors(PR.base_anchors(s, scales, ratios), H, W, (s, s)) for (H, W), s in zip(sizes, strides)])
    cls = [BC.f32(rng.normal(0, 1.5, (BATCH, A, H, W))) for H, W in sizes]
    reg = []
    for H, W in sizes:
        r = rng.normal(0.0, 0.3, (BATCH, A, 6, H, W))
        r[:, :, 4:] = rng.uniform(-0.95, 0.95, (BATCH, A, 2, H, W))
        reg.append(BC.f32(r.reshape(BATCH, 6 * A, H, W)))
    counts = [H * W * A for H, W in sizes]
    keep_counts = [7] if len(sizes) == 1 else [5, 0, counts[2]]
    keep = [[rng.permutation(n)[:k] for n, k in zip(counts, keep_counts)] for _ in range(BATCH)]
    return dict(A=A, sizes=sizes, priors=priors, cls=cls, reg=reg, keep_counts=keep_counts, keep=keep)


def prop_ref(c, b, dtype=F64):
    return PR.decode_kept([m[b] for m in c["cls"]], [m[b] for m in c["reg"]], c["priors"], c["sizes"], c["A"], c["keep"][b], PC.MEANS, PC.STDS, dtype)


def prop_condition(c):
    for b in range(BATCH):
        _, rb, _, _ = prop_ref(c, b)
        w, h, t = rb[:, 2], rb[:, 3], rb[:, 4]
        if (np.abs(w - h) < SHAPE_GAP * np.maximum(w, h)).any() or (np.abs(np.abs(t) - np.pi / 2) < SHAPE_GAP).any():
            return False
        if (np.abs(w - PROP_MIN_SIZE) < SHAPE_GAP).any() or (np.abs(h - PROP_MIN_SIZE) < SHAPE_GAP).any():
            return False
        ok = (w > PROP_MIN_SIZE) & (h > PROP_MIN_SIZE)
        if not 0 < ok.sum() < len(ok):      # min_bbox_size removes some and not all
            return False
    return True


PROP_SEEDS = {}


@functools.lru_cache(maxsize=None)
def prop_case(name):
    return _prop_try(name, PROP_SEEDS[name])


# ------------------------------------------------------------------------------------------------------------------- the committed seeds
GEOM_SEEDS.update({(1, 1, True): 0, (7, 1, True): 0, (7, 3, True): 0, (7, 3, False): 0, (3, 2, True): 0, (3, 2, False): 0, (14, 2, True): 3, (8, 4, False): 1,
                   (16, 2, True): 1, (32, 1, False): 1})
LOSS_SEEDS.update({(S, B, K): 0 for S, B, K, _ in LOSS_CASES})
PREDICT_SEEDS.update({(n, K): 0 for n, K, _ in PREDICT_CASES})
PROP_SEEDS.update({"A1": 81, "A9": 1, "single": 29})


def find_seeds():
    return dict(GEOM=dict((g, BC.first_seed(_geom_try, lambda r, g=g: geom_condition(r, *g))) for g in GEOMS),
                PIXEL=BC.first_seed(_pixel_try, pixel_condition), CLAMP=BC.first_seed(lambda s: s, clamp_condition),
                LOSS=dict(((S, B, K), BC.first_seed(lambda s, a=(S, B, K): _loss_try(*a, s), loss_condition)) for S, B, K, _ in LOSS_CASES),
                PREDICT=dict(((n, K), BC.first_seed(lambda s, a=(n, K): _predict_try(*a, s), lambda c, n=n: predict_condition(c, n))) for n, K, _ in PREDICT_CASES),
                PROP=dict((n, BC.first_seed(lambda s, n=n: _prop_try(n, s), prop_condition)) for n in PROP_SHAPES))


if __name__ == "__main__":      # prints the first passing seeds
    print(find_seeds())
