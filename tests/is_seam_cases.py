"""Input sets of the seam tests of the instance-segmentation kernels (csrc/mask_head.hip, csrc/hbox_head.hip) and the conditions they must meet,
from the float64 restatements (mask_ref, hbox_ref) alone.  Plain helper module: no tests, no fixtures.  tests/test_is_seams_host.py asserts every
condition on the CPU, tests/test_hip_is_seams.py runs the kernels on the same inputs.  The sizes are the smallest that cross each seam:
  1. RoIAlign chunks: R = 130 RoIs (trips of 64, 64 and 2 in the backward's walk), C up to 257 (four registers per lane, a second channel chunk),
     82 map pixels whose image and level boundaries fall inside a workgroup of four pixel keys;
  2. RoIAlign sizes: out_size 1 .. 32, fixed grids of 8, 9 and 64, caller-given levels outside [0, n), image indices that name no image;
  3. the mask loss: M M on either side of the 256 threads, 99 slots (a second trip of the 64 lanes of the sum), n_pos outside [0, S];
  4. the paste: a zero-width box on a pixel centre (0 / 0);
  5. the box half: sample lists of more than one 256-slot chunk, more than 64 partial rows, proposals over more than one workgroup.
Every float is compared with `held`: the kernel's error against float64 below 4 x the error of the float32 CPU restatement against float64,
floor 1e-6.  Thresholds decide bits, so the seeds are the first that keep every float64 value clear of them (python tests/is_seam_cases.py prints
the seeds); the host test asserts the margins again."""
import functools

import numpy as np

import box_cases as BC
import hbox_cases as HC
import hbox_ref as HR
import mask_cases as MC
import mask_ref as MR
import rpn_ref
from conftest import record_parity

F64, F32 = np.float64, np.float32


def err_of(a, ref):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return float(np.abs(a.astype(F64) - ref).max()) if ref.size else 0.0


def bound_of(ref64, ref32):
    """the bound of `held` and the float32 error it comes from"""
    e32 = err_of(np.asarray(ref32), np.asarray(ref64, F64))
    return max(4 * e32, 1e-6), e32


def held(tag, out, ref64, ref32):
    """the rule of tests/test_hip_mask.py and tests/test_hip_hbox.py: 4 x the float32 CPU error of the restatement against float64, floor 1e-6"""
    ref64 = np.asarray(ref64, F64)
    err = err_of(out, ref64)
    bound, e32 = bound_of(ref64, ref32)
    record_parity("is_seams", tag, err)
    record_parity("is_seams", "ref_f32_cpu_" + tag, e32)
    print("%s: err %.3e, float32 restatement %.3e" % (tag, err, e32))
    assert tuple(out.shape) == ref64.shape and err < bound, (tag, err, e32)


def bin_major(x):
    """(R, C, P, P) -> the kernels' (R, P P, C)"""
    return np.ascontiguousarray(np.transpose(x.reshape(x.shape[0], x.shape[1], -1), (0, 2, 1)))


def rows_of(maps, ld):
    """NCHW maps -> per level (N H W, ld) rows whose first C columns are the channels, the rest zeros"""
    out = []
    for m in maps:
        N, Cc, H, W = m.shape
        r = np.zeros((N * H * W, ld), F32)
        r[:, :Cc] = np.transpose(m, (0, 2, 3, 1)).reshape(-1, Cc)
        out.append(r)
    return out


def nchw_of(rows, shape):
    N, Cc, H, W = shape
    return np.transpose(rows[:, :Cc].reshape(N, H, W, Cc), (0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------------------------- 1. RoIAlign chunks
# Two images, two levels of 7 x 5 (stride 8) and 3 x 2 (stride 16): 2 * 35 + 2 * 6 = 82 pixel keys in (level, image, y, x) order.  Image 1 of level
# 0 starts at key 35 and level 1 at key 70, neither a multiple of the 4 keys of a workgroup; the 21st workgroup has keys 80 and 81 and two idle
# waves.  The RoIs named in AL_NAMED sit on the first and last lane of the three trips of the backward's walk, lie on image 0, level 0 and cover
# pixel AL_PIXEL; their dout is positive, so that each puts a weight on that pixel in every channel that no rounding could hide.  RoIs 65 .. 126 lie
# on image 1: for a pixel of image 1 the first trip has no hit and the second is full of candidates.
AL_IMAGES, AL_SIZES, AL_STRIDES, AL_OUT, AL_R, AL_FINEST = 2, ((7, 5), (3, 2)), (8, 16), 14, 130, 56.0
AL_SCALES = [1.0 / s for s in AL_STRIDES]
AL_C, AL_CMAX = (1, 64, 65, 256, 257), 257
AL_NAMED, AL_PIXEL = (0, 63, 64, 127, 128, 129), (3, 2)      # pixel (y, x)
AL_VALID_C, AL_PER_GROUP, AL_COUNTS = 65, 26, (26, 0, 13, 26, 25)
AL_SEED = 1


@functools.lru_cache(maxsize=None)
def align_case():
    """dict: feats [(2, 257, H, W)], rois (130, 5), levels (130) int32, dout (130, 257, 14, 14).  A case of C channels takes the first C of them: no
    operation of RoIAlign mixes channels, so its reference is the first C channels of the reference at 257 (the host test holds that)."""
    rng = np.random.default_rng(AL_SEED)
    feats = [rng.standard_normal((AL_IMAGES, AL_CMAX, H, W)).astype(F32) for H, W in AL_SIZES]
    ctr = np.stack([rng.uniform(2, 38, AL_R), rng.uniform(2, 54, AL_R)], 1)      # the image is 40 wide and 56 tall; some boxes reach outside
    wh = rng.uniform(5, 44, (AL_R, 2))
    rois = np.zeros((AL_R, 5), F32)
    rois[:, 1:] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    rois[65:127, 0] = 1
    levels = rng.integers(0, len(AL_SIZES), AL_R).astype(np.int32)
    dout = rng.standard_normal((AL_R, AL_CMAX, AL_OUT, AL_OUT)).astype(F32)
    for r in AL_NAMED:
        c, s = np.array([20.0, 28.0]) + rng.uniform(-2, 2, 2), rng.uniform(10, 26, 2)      # pixel (3, 2) of the stride-8 map is x 16 .. 24, y 24 .. 32
        rois[r] = np.concatenate([[0.0], c - s / 2, c + s / 2])
        levels[r] = 0
        dout[r] = np.abs(dout[r]) + F32(0.5)
    return dict(feats=feats, rois=rois, levels=levels, dout=dout)


def align_in_use(kind):
    """'all': every slot; 'valid': slot r is in use iff r % 26 < AL_COUNTS[r // 26]"""
    r = np.arange(AL_R)
    return np.ones(AL_R, bool) if kind == "all" else (r % AL_PER_GROUP) < np.asarray(AL_COUNTS)[r // AL_PER_GROUP]


def _align_run(Cc, use, ft, what):
    c = align_case()
    feats = [f[:, :Cc] for f in c["feats"]]
    if what == "fwd":
        return MR.roi_align(feats, c["rois"], AL_STRIDES, AL_OUT, 0, True, AL_FINEST, levels=c["levels"], in_use=use, ft=ft)[0]
    return MR.roi_align_bwd(c["dout"][:, :Cc], [f.shape for f in feats], c["rois"], AL_STRIDES, AL_OUT, 0, True, AL_FINEST, levels=c["levels"], in_use=use, ft=ft)


@functools.lru_cache(maxsize=None)
def align_refs(kind):
    """dict(fwd64, fwd32 (130, C, 14, 14), bwd64, bwd32 [per level (2, C, H, W)]) with C = 257 for 'all' and 65 for 'valid'; computed once, never
    modified: the tests slice the channels they run"""
    Cc, use = (AL_CMAX, None) if kind == "all" else (AL_VALID_C, align_in_use("valid"))
    return dict(fwd64=_align_run(Cc, use, F64, "fwd"), fwd32=_align_run(Cc, use, F32, "fwd"), bwd64=_align_run(Cc, use, F64, "bwd"),
                bwd32=_align_run(Cc, use, F32, "bwd"))


@functools.lru_cache(maxsize=None)
def align_without(r, kind="all"):
    """the float64 gradient of level 0 with RoI r taken out of use, at pixel AL_PIXEL of image 0 -> (C)"""
    Cc = AL_CMAX if kind == "all" else AL_VALID_C
    use = align_in_use(kind).copy()
    use[r] = False
    return _align_run(Cc, use, F64, "bwd")[0][0, :, AL_PIXEL[0], AL_PIXEL[1]].copy()


# ------------------------------------------------------------------------------------------------------------------- 2. RoIAlign sizes
# Nine RoIs on the first five channels of the maps above: inside, reaching out on every side, larger than the image (an adaptive grid of 9 at
# out_size 1: beyond the dense walk), thin, of zero width.
SZ_C, SZ_SEED = 5, 3
SZ_ROIS = np.array([[0, 4.2, 6.1, 30.7, 41.3], [1, -7.5, -5.2, 18.4, 22.9], [0, 21.3, 30.6, 52.8, 66.1], [1, -12.0, -9.0, 58.0, 61.0], [0, 3.1, 20.4, 37.9, 24.2],
                    [1, 17.5, 8.0, 17.5, 40.0], [0, 10.4, 12.3, 26.2, 47.7], [1, 1.8, 2.6, 12.1, 10.9], [0, 14.9, 25.2, 35.0, 50.3]], F32)
SZ_LEVELS = np.array([0, 1, 0, 0, 1, 0, 1, 0, 1], np.int32)
SZ_OUT_CASES = [(P, s) for P in (1, 2, 31, 32) for s in (0, 2)]
SZ_GRID_CASES = [(P, s) for s in (8, 9, 64) for P in (2, 7)]      # the dense walk's last value, its first non-dense value and the cap
SZ_BAD_LEVELS = np.array([0, -1, len(AL_SIZES) + 3, 0, 1, -7, 1, 0, 1], np.int32)      # the kernels clamp them to [0, n)
SZ_BAD_IMAGES = {2: -1.0, 4: 2.0, 7: np.nan}      # slot -> an image index that names no image: a zero row, level -1, no gradient


def size_feats():
    return [f[:, :SZ_C] for f in align_case()["feats"]]


def size_dout(P, scale=1.0):
    return (np.random.default_rng(SZ_SEED + P).standard_normal((len(SZ_ROIS), SZ_C, P, P)) * scale).astype(F32)


def bad_image_rois():
    rois = SZ_ROIS.copy()
    for r, b in SZ_BAD_IMAGES.items():
        rois[r, 0] = b
    return rois


def size_refs(rois, levels, P, sampling, dout):
    """-> (fwd64, fwd32, bwd64, bwd32) of the nine RoIs"""
    feats = size_feats()
    shapes = [f.shape for f in feats]
    out = []
    for ft in (F64, F32):
        out.append(MR.roi_align(feats, rois, AL_STRIDES, P, sampling, True, AL_FINEST, levels=levels, ft=ft)[0])
    for ft in (F64, F32):
        out.append(MR.roi_align_bwd(dout, shapes, rois, AL_STRIDES, P, sampling, True, AL_FINEST, levels=levels, ft=ft))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------- 3. the mask loss
# (a) the mask size: mask_cases' 'base' layout (K = 3, 16 slots) at M = 1, 2 (far below the 256 threads), 16 (M M = 256 exactly) and 17 (just past).
ML_SIZES = (1, 2, 16, 17)
ML_SEEDS = {1: 100, 2: 100, 16: 101, 17: 105}      # the first seeds of the 'base' builder from 100 that pass avg_margin (size_seed)
ML_TRIES = 30


def slot_refs(c, z, n_pos, M, loss_weight=MC.LOSS_WEIGHT):
    """mask_ref on the fixed slots of a case (boxes, sample_gt (B, S), labels, bitmaps) with logits z (B S, K, M, M) -> (use, float64, float32):
    dict(avg, targets, loss (1), slot, d)"""
    B, S = c["sample_gt"].shape
    use = (np.arange(S)[None, :] < np.asarray(n_pos)[:, None]).reshape(-1)
    out = []
    for ft in (F64, F32):
        avg, tg = np.zeros((B * S, M, M), ft), np.zeros((B * S, M, M), np.uint8)
        if use.any():
            avg[use], tg[use] = MR.mask_targets(c["boxes"][use], c["sample_gt"].reshape(-1)[use], c["bitmaps"], M, ft=ft)
        loss, slot, d = MR.mask_loss(z, tg, np.where(use, c["labels"], -1), int(np.sum(n_pos)), loss_weight, ft)
        out.append(dict(avg=avg, targets=tg, loss=np.asarray([loss]), slot=slot, d=d))
    return use, out[0], out[1]


def avg_margin(c, n_pos, M):
    """the smallest float64 distance of a target average of a slot in use from 0.5"""
    B, S = c["sample_gt"].shape
    use = (np.arange(S)[None, :] < np.asarray(n_pos)[:, None]).reshape(-1)
    avg, _ = MR.mask_targets(c["boxes"][use], c["sample_gt"].reshape(-1)[use], c["bitmaps"], M)
    return float(np.abs(avg - 0.5).min())


def loss_logits(n, K, M, seed):
    return (np.random.default_rng(seed).standard_normal((n, K, M, M)) * 2.0).astype(F32)


@functools.lru_cache(maxsize=None)
def size_case(M):
    return MC.build("base", ML_SEEDS[M])


def size_seed(M):
    """mask_cases.search() at mask size M: the first seed of the 'base' builder from 100 whose target averages keep MARGIN from 0.5"""
    for seed in range(100, 100 + ML_TRIES):
        c = MC.build("base", seed)
        if avg_margin(c, c["n_pos"], M) > MC.MARGIN:
            return seed
    raise RuntimeError("no seed at M = %d" % M)


# (b) the slot count: 3 images x 33 slots at M = 28, at most 4 positives per image; image 2's slots are 66 .. 98, the second trip of the sum's lanes
SL_B, SL_S, SL_NPOS, SL_GTS = 3, 33, (4, 3, 4), 2
SL_SEED = 1      # the first that passes slots_condition


def _slots_try(seed):
    rng = np.random.default_rng(3100 + seed)
    bitmaps, gt_boxes = zip(*[MC.blob(rng) for _ in range(SL_B * SL_GTS)])
    boxes = rng.uniform(0, MC.IMG / 2, (SL_B, SL_S, 4)).astype(F32)
    boxes[:, :, 2:] += boxes[:, :, :2] + 4
    sample_gt, labels = np.full((SL_B, SL_S), -1, np.int64), np.zeros((SL_B, SL_S), np.int64)
    gt_labels = rng.integers(0, MC.K, SL_B * SL_GTS)
    for b in range(SL_B):
        for j in range(SL_NPOS[b]):
            g = b * SL_GTS + j % SL_GTS
            boxes[b, j] = gt_boxes[g] + rng.uniform(-3.0, 3.0, 4).astype(F32) * (j >= SL_GTS)      # the gt's own box, then jittered ones
            sample_gt[b, j], labels[b, j] = g, gt_labels[g]
    return dict(bitmaps=np.stack(bitmaps), boxes=boxes.reshape(-1, 4), sample_gt=sample_gt, labels=labels.reshape(-1), n_pos=np.asarray(SL_NPOS, np.int64),
                logits=loss_logits(SL_B * SL_S, MC.K, MC.M, 31 + seed))


def slots_condition(c):
    return avg_margin(c, c["n_pos"], MC.M) > MC.MARGIN


@functools.lru_cache(maxsize=None)
def slots_case():
    return _slots_try(SL_SEED)


# (c) n_pos outside [0, S]: 'base' with its last slot of image 0 filled, so that all S slots of image 0 name a gt; the device is handed [S + 5, -3]
CLAMP_GIVEN = (MC.S + 5, -3)
CLAMP_MEANT = (MC.S, 0)


@functools.lru_cache(maxsize=None)
def clamp_case():
    c = dict(MC.case("base"))
    sg, labels, boxes = c["sample_gt"].copy(), c["labels"].copy(), c["boxes"].copy()
    sg[0, MC.S - 1] = 0
    labels[MC.S - 1] = c["gt_labels"][0]
    boxes[MC.S - 1] = c["gt_boxes"][0] + np.array([1.5, -2.0, 2.5, 1.0], F32)
    c.update(sample_gt=sg, labels=labels, boxes=boxes)
    return c


# ------------------------------------------------------------------------------------------------------------------- 4. the paste: 0 / 0
PASTE_NAN_ROW, PASTE_NAN_X = 3, 10.5      # instance 3 has x1 = x2 = 10.5: pixel column 10 is 0 / 0, every other column +-inf, which maps to 0


def paste_case():
    """(logits, labels, boxes, h, w) of mask_cases' 'base' paste, its zero-width box moved onto the centre of pixel column 10"""
    p = MC.case("base")["paste"]
    boxes = p["boxes"].copy()
    boxes[PASTE_NAN_ROW] = [PASTE_NAN_X, 8.0, PASTE_NAN_X, 30.0]
    return p["logits"], p["labels"], boxes, MC.PASTE_HW[0], MC.PASTE_HW[1]


# ------------------------------------------------------------------------------------------------------------------- 5a. the RPN loss over chunks
# hbox_cases' pyramid (1023 anchors), two images, S slots each of distinct anchors (the gradients are plain stores: a repeated anchor would be a
# race of the test's making).  The positives come first in a slot list, so a positive in every 256-slot chunk of image 1 at S = 520 means that
# image 1 is nearly all positives there; everywhere else a quarter of the slots are.  Image 0 uses fewer than S slots.
RL_S = (256, 257, 520)
RL_SEEDS = {256: 0, 257: 0, 520: 1}      # the first seeds that pass rpn_loss_condition
RL_CHUNK = 256


def rpn_loss_counts(S):
    n_pos = np.array([S // 4, 516 if S == 520 else S // 4], np.int64)
    return n_pos, np.array([S - n_pos[0] - 5, S - n_pos[1]], np.int64)


def _rpn_loss_try(S, seed):
    rng = np.random.default_rng(3200 + 1000 * S + seed)
    cls = [BC.f32(rng.normal(0.0, 1.5, (HC.BATCH, HC.A, H, W))) for H, W in HC.SIZES]
    reg = [BC.f32(rng.normal(0.0, 0.4, (HC.BATCH, 4 * HC.A, H, W))) for H, W in HC.SIZES]
    pr = HC.priors(F32)
    firsts = np.cumsum([0] + [h * w * HC.A for h, w in HC.SIZES])
    n_pos, n_neg = rpn_loss_counts(S)
    samples, gts = np.zeros((HC.BATCH, S), np.int64), []
    for b in range(HC.BATCH):
        forced = np.array([rng.integers(firsts[l], firsts[l + 1]) for l in range(len(HC.SIZES))])      # every level has a sample
        rest = np.setdiff1d(np.arange(len(pr)), forced)
        idx = np.concatenate([forced, rest[rng.permutation(len(rest))[:S - len(forced)]]])
        idx = idx[np.concatenate([rng.permutation(int(n_pos[b] + n_neg[b])), np.arange(n_pos[b] + n_neg[b], S)])]      # ... among the slots in use
        samples[b] = idx
        p = pr[idx[:n_pos[b]]].astype(F64)      # each positive's gt: its anchor, jittered
        ctr, wh = (p[:, :2] + p[:, 2:]) / 2, p[:, 2:] - p[:, :2]
        ctr, wh = ctr + rng.uniform(-0.12, 0.12, ctr.shape) * wh, wh * rng.uniform(0.8, 1.25, wh.shape)
        gts.append(BC.f32(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)))
    return dict(S=S, cls=cls, reg=reg, samples=samples, gts=gts, n_pos=n_pos, n_neg=n_neg)


def rpn_loss_lists(c):
    """the lists as hbox_ref.rpn_loss takes them: per image (pos, pos_gt, neg)"""
    return [(c["samples"][b, :p], np.arange(p), c["samples"][b, p:p + n]) for b, (p, n) in enumerate(zip(c["n_pos"], c["n_neg"]))]


def rpn_loss_refs(c):
    """(float64, float32) of hbox_ref.rpn_loss: (loss_cls (L), loss_bbox (L), dcls[l], dreg[l], targets per image)"""
    ls = rpn_loss_lists(c)
    return tuple(HR.rpn_loss(c["cls"], c["reg"], HC.SIZES, HC.A, HC.priors(F32), c["gts"], [l[0] for l in ls], [l[1] for l in ls], [l[2] for l in ls],
                             HC.RPN_MEANS, HC.RPN_STDS, dtype=ft) for ft in (F64, F32))


def rpn_l1_terms(c, r64):
    """per image the positives' own L1 terms |pred - target| (n_pos, 4) in float64"""
    out = []
    for b, (pos, _, _) in enumerate(rpn_loss_lists(c)):
        lvl, y, x, a = rpn_ref.level_of(pos, HC.SIZES, HC.A)
        pred = np.stack([c["reg"][l][b, an * 4:an * 4 + 4, yy, xx] for l, yy, xx, an in zip(lvl, y, x, a)]).astype(F64)
        out.append(np.abs(pred - r64[4][b]))
    return out


def rpn_chunk_terms(c, r64):
    """per 256-slot chunk of image 1 the largest share a positive of the chunk has in loss_bbox: its four L1 terms / avg_factor"""
    terms = rpn_l1_terms(c, r64)[1].sum(1) / float((c["n_pos"] + c["n_neg"]).sum())
    return [float(terms[k:k + RL_CHUNK].max()) if len(terms) > k else 0.0 for k in range(0, c["S"], RL_CHUNK)]


def rpn_loss_condition(c):
    r64, r32 = rpn_loss_refs(c)
    if min(float(t.min()) for t in rpn_l1_terms(c, r64)) <= HC.THR_GAP:      # the sign of an L1 term is the gradient
        return False
    for b, (pos, _, neg) in enumerate(rpn_loss_lists(c)):
        if len(np.unique(c["samples"][b])) != c["S"] or set(rpn_ref.level_of(np.concatenate([pos, neg]), HC.SIZES, HC.A)[0].tolist()) != set(range(len(HC.SIZES))):
            return False
    if c["S"] == 520 and not min(rpn_chunk_terms(c, r64)) > 100 * bound_of(r64[1], r32[1])[0]:
        return False
    return True


@functools.lru_cache(maxsize=None)
def rpn_loss_case(S):
    return _rpn_loss_try(S, RL_SEEDS[S])


# ------------------------------------------------------------------------------------------------------------------- 5b. the RoI loss over partial rows
# test_hip_hbox.seam_case's recipe with the images, the slots and the counts given: the kernel runs one wave per row and four rows per workgroup, so
# row r lands in partial row r // 4, and the sum's lane i adds partial rows i, i + 64, ...  The positives come first in an image's slots; the counts
# put one in a row >= 256 in every case (the host test asserts it).
RS_CASES = {(1, 257, 3): ((257,), (0,)), (2, 130, 3): ((43, 128), (87, 0)), (2, 512, 3): ((170, 170), (342, 340)), (2, 130, 80): ((43, 128), (87, 0))}
RS_SEEDS = {k: 0 for k in RS_CASES}      # the first seeds that pass roi_loss_condition


def _roi_loss_try(B, S, K, seed):
    rng = np.random.default_rng(3300 + 7 * S + K + 1000 * seed)
    n, G = B * S, 5
    c, wh = rng.uniform(16, 48, (G, 2)), rng.uniform(10, 30, (G, 2))
    gts = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    gt_labels = rng.integers(0, K, G).astype(np.int64)
    gt_labels[0] = K - 1      # the last class: the last 16 bytes of a row of deltas
    n_pos, n_neg = (np.asarray(v, np.int64) for v in RS_CASES[(B, S, K)])
    sgt = -np.ones((B, S), np.int64)
    for b in range(B):
        sgt[b, :n_pos[b]] = rng.integers(0, G, n_pos[b])
    sgt[0, 0] = 0
    rois = np.zeros((n, 5), F32)
    rois[:, 0] = np.repeat(np.arange(B), S)
    ctr, rwh = rng.uniform(16, 48, (n, 2)), rng.uniform(8, 30, (n, 2))
    rois[:, 1:] = np.concatenate([ctr - rwh / 2, ctr + rwh / 2], 1)
    for b in range(B):      # a positive's RoI lies on its gt, as the assigner sees to: the encoded targets are O(1)
        for j in range(n_pos[b]):
            rois[b * S + j, 1:] = gts[sgt[b, j]] + rng.uniform(-1.5, 1.5, 4)
    cls = rng.normal(0, 2.0, (n, K + 1)).astype(F32)
    reg = rng.normal(0, 0.5, (n, 4 * K)).astype(F32)
    return cls, reg, dict(rois=rois, sample_gt=sgt, n_pos=n_pos, n_neg=n_neg, gts=gts, gt_labels=gt_labels)


def roi_loss_refs(cls, reg, K, s, reg_target):
    return tuple(HR.roi_loss(cls, reg, K, s["rois"][:, 1:], s["gts"], s["gt_labels"], s["sample_gt"], s["n_pos"], s["n_neg"], HC.ROI_MEANS, HC.ROI_STDS, reg_target,
                             dtype=ft) for ft in (F64, F32))


def roi_loss_condition(case):
    """no L1 term within THR_GAP of its target under either regression target; no two logits that decide a top-1 hit closer than SCORE_GAP"""
    cls, reg, s = case
    K = cls.shape[1] - 1
    for t in ("reference", "encoded"):
        r = HR.roi_loss(cls, reg, K, s["rois"][:, 1:], s["gts"], s["gt_labels"], s["sample_gt"], s["n_pos"], s["n_neg"], HC.ROI_MEANS, HC.ROI_STDS, t)
        rows = np.nonzero((r["labels"] >= 0) & (r["labels"] < K))[0]
        pred = np.stack([reg[q, 4 * r["labels"][q]:4 * r["labels"][q] + 4] for q in rows])
        if not HR.l1_margin(pred, r["targets"][rows]) > HC.THR_GAP:
            return False
    z = np.sort(cls.astype(F64), 1)
    return bool((z[:, -1] - z[:, -2] > HC.SCORE_GAP).all())


@functools.lru_cache(maxsize=None)
def roi_loss_case(B, S, K):
    return _roi_loss_try(B, S, K, RS_SEEDS[(B, S, K)])


# ------------------------------------------------------------------------------------------------------------------- 5c. proposals over workgroups
# nms_pre 100 on hbox_cases' planted maps keeps 100 + 100 + 48 + 12 + 3 = 263 anchors per image: 526 slots, three workgroups of 256 threads, the
# image boundary (263) inside the second and a level's keep_first (100, 200, 248, 260 and 363, 463, 511, 523) inside every one.
PROP_NMS_PRE, PROP_MIN_SIZES = 100, (0.0, 6.0)


def proposal_keep(cls):
    """per image the kept anchors of every level; the counts per level"""
    keep = [rpn_ref.topk_per_level([m[b] for m in cls], PROP_NMS_PRE) for b in range(cls[0].shape[0])]
    return keep, [len(k) for k in keep[0]]


def proposal_refs(cls, reg, keep):
    """per image ((scores, boxes, level ids) float64, the same float32)"""
    out = []
    for b in range(cls[0].shape[0]):
        args = ([m[b] for m in cls], [m[b] for m in reg], HC.priors(F32), HC.SIZES, HC.A, keep[b], HC.RPN_MEANS, HC.RPN_STDS, HC.IMG)
        out.append((HR.rpn_decode_kept(*args, dtype=F64), HR.rpn_decode_kept(*args, dtype=F32)))
    return out


def proposal_size_condition(cls, reg, keep, min_size):
    """hbox_cases' condition on the size flag: no clipped width or height within THR_GAP of min_size, other than the exact zero of a box THR_GAP
    clear outside the image"""
    for b in range(cls[0].shape[0]):
        cb, rb = [m[b] for m in cls], [m[b] for m in reg]
        bx = HR.rpn_decode_kept(cb, rb, HC.priors(), HC.SIZES, HC.A, keep[b], HC.RPN_MEANS, HC.RPN_STDS, HC.IMG)[1]
        raw = HR.rpn_decode_kept(cb, rb, HC.priors(), HC.SIZES, HC.A, keep[b], HC.RPN_MEANS, HC.RPN_STDS, None)[1]
        wh = np.stack([bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]], 1)
        out = np.stack([(raw[:, 0] > HC.IMG[1] + HC.THR_GAP) | (raw[:, 2] < -HC.THR_GAP), (raw[:, 1] > HC.IMG[0] + HC.THR_GAP) | (raw[:, 3] < -HC.THR_GAP)], 1)
        near = np.abs(wh - min_size) < HC.THR_GAP
        if (near & ~((wh == 0) & out & (min_size == 0))).any():
            return False
    return True


if __name__ == "__main__":      # prints the first passing seeds
    print("ML_SEEDS", {M: size_seed(M) for M in ML_SIZES})
    print("SL_SEED", BC.first_seed(_slots_try, slots_condition))
    print("RL_SEEDS", {S: BC.first_seed(lambda s, S=S: _rpn_loss_try(S, s), rpn_loss_condition) for S in RL_S})
    print("RS_SEEDS", {k: BC.first_seed(lambda s, k=k: _roi_loss_try(k[0], k[1], k[2], s), roi_loss_condition) for k in RS_CASES})
