"""GPU: sliding-window segmentation inference and the IoU metric on the kernels of csrc/seg_eval.hip, every buffer out of a guard.Arena (poisoned
outputs, guards on both sides, frozen inputs, the wrappers' own allocations included).
  * window accumulate in exact arithmetic (integer logits, scale 4: every product and sum is exact in f32) bit for bit against the torch loop, f32 and
    bf16 inputs; the division and the arg-max on the same data, ties included;
  * arg-max: padding columns that would win, K = 2, K = 150 with an accumulator pitch larger than Kp;
  * areas: bit-exact against the reference formulas (torch.histc on the masked maps) for K = 2, 7, 37, 150, uint8 and int64 labels, a ragged 37 x 53
    map, an all-ignored map, accumulation over calls, counters preset to 2^40, two runs identical;
  * real-valued logits: the prediction equals the float64 torch restatement wherever the reference's top-2 gap exceeds 1e-4 * max(1, max |logit|);
  * end to end: EncoderDecoder.predict (slide and whole mode, padding and ori_shape) + IoUMetric against the torch loop on the very same per-window
    low-resolution logits."""
import functools

import pytest
import torch
import torch.nn.functional as F

import guard
import seg_eval_ref as R
from conftest import rel_err
from mtp_amd import ops

pytestmark = pytest.mark.gpu
F32, BF16, U8, I64 = torch.float32, torch.bfloat16, torch.uint8, torch.int64
IMG, CROP, STRIDE = (56, 88), (32, 48), (24, 32)      # fixture f18's geometry 'a': column origins 0, 32, 40 (the last clamped), counts {1, 2, 3, 4, 6}
N, K = 2, 7
GAP, CAP = 1e-4, 0.005                                 # the real-valued rule: pixels under the gap are excluded, at most 0.5 % of them may be

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


def e(*shape, dtype=F32):
    return ARENA.empty(*shape, dtype=dtype)


def rows(lr, dtype=F32):
    """(N, K, h, w) logits -> the head's rows (N*h*w, Kp) on the device, columns K .. Kp zero: an op INPUT, frozen"""
    n, k, h, w = lr.shape
    r = torch.zeros(n * h * w, ops.pad8(k))
    r[:, :k] = lr.permute(0, 2, 3, 1).reshape(-1, k)
    return ARENA.frozen(ARENA.like(r, dtype=dtype))


def nchw(acc, k):
    return acc[..., :k].cpu().permute(0, 3, 1, 2).contiguous()


def counts(H, W, crop, stride):
    from mtp_amd.segmentors.encoder_decoder import window_counts
    return ARENA.frozen(window_counts(H, crop[0], stride[0]).cuda()), ARENA.frozen(window_counts(W, crop[1], stride[1]).cuda())


def accumulate(low, dtype, k=K):
    """the window loop on the device -> acc (N, H, W, Kp)"""
    wins, _ = R.slide_windows(*IMG, CROP, STRIDE)
    acc = ARENA.zeros(low[0].shape[0], *IMG, ops.pad8(k))
    for (y1, x1), lr in zip(wins, low):
        ops.seg_window_accumulate(rows(lr, dtype), k, lr.shape[0], lr.shape[2], lr.shape[3], acc, y1, x1, *CROP)
    return acc


def top2_gap(seg):
    t = seg.topk(2, dim=1).values
    return t[:, 0] - t[:, 1]


def sure_pixels(seg_ref):
    """(mask of pixels whose reference top-2 gap exceeds the threshold, fraction under it): the cap is asserted on the reference first"""
    sure = top2_gap(seg_ref) > GAP * max(1.0, seg_ref.abs().max().item())
    frac = 1.0 - sure.double().mean().item()
    assert frac <= CAP, "the reference itself has %.3f %% of pixels under the gap" % (100 * frac)
    return sure, frac


def areas_of(pred, lab, k):
    return sum(R.torch_areas(pred[i].long(), lab[i].long(), k) for i in range(pred.shape[0]))


# ------------------------------------------------------------------------------------------------ exact arithmetic
@functools.lru_cache(maxsize=None)
def exact_case():
    g = torch.Generator().manual_seed(56088)
    wins, _ = R.slide_windows(*IMG, CROP, STRIDE)
    low = [torch.randint(-8, 9, (N, K, CROP[0] // 4, CROP[1] // 4), generator=g).float() for _ in wins]
    seg, preds, _ = R.torch_slide_from_lowres(low, CROP, STRIDE, *IMG)
    assert torch.equal(preds.double(), R.torch_slide_from_lowres([x.double() for x in low], CROP, STRIDE, *IMG)[1])      # torch's f32 sums are exact too
    return low, seg, preds


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_window_accumulate_divide_argmax_exact(dtype):
    """integers in [-8, 8] and scale 4: the weights are multiples of 1 / 8, every product and sum is exact in f32 (and the inputs in bf16), so the
    accumulator equals torch's bit for bit whatever the order.  The division: counts 1, 2, 4 are powers of two; 3 and 6 also occur at this geometry
    (column origins 0, 32, 40) -- a correctly rounded quotient of an exact numerator, the same in torch and in the kernel"""
    low, seg, preds = exact_case()
    acc = accumulate(low, dtype)
    assert torch.equal(nchw(acc, K), preds)
    assert acc[..., K:].abs().max().item() == 0.0
    ARENA.frozen(acc)                                                               # the arg-max pass must not write it
    cy, cx = counts(*IMG, CROP, STRIDE)
    pred, out = e(N, *IMG, dtype=U8), e(N, K, *IMG)
    ops.seg_argmax_areas(acc, K, cy, cx, pred=pred, seg_logits=out)
    assert torch.equal(out.cpu(), seg)
    ties = (top2_gap(seg) == 0).double().mean().item()
    assert ties > 0.001, "no ties in the data: the first-index rule is not exercised"
    assert torch.equal(pred.cpu().long(), seg.argmax(dim=1))
    ARENA.check()
    # write_back: the divided rows in place (what predict() resizes when ori_shape differs)
    acc2 = ARENA.like(acc)
    ops.seg_argmax_areas(acc2, K, cy, cx, write_back=True)
    assert torch.equal(nchw(acc2, K), seg)


# ------------------------------------------------------------------------------------------------ arg-max
def test_argmax_ignores_padding_columns_that_would_win():
    """all logits negative, K = 7: the zero (or anything larger) in column 7 of the padded row would win if it took part"""
    H, W = 37, 53
    g = torch.Generator().manual_seed(7)
    a = torch.zeros(N, H, W, 8)
    a[..., :7] = -0.1 - torch.rand(N, H, W, 7, generator=g)
    a[0, :, :, 7] = 1e30
    acc = ARENA.frozen(ARENA.like(a))
    pred = ops.seg_argmax_areas(acc, 7, pred=e(N, H, W, dtype=U8))
    assert int(pred.max()) <= 6 and torch.equal(pred.cpu().long(), a[..., :7].argmax(dim=3))


@pytest.mark.parametrize("k,pitch", [(2, 8), (150, 160), (256, 256)])
def test_argmax_two_classes_and_many_classes_with_a_wider_pitch(k, pitch):
    """K = 150: Kp = 152 inside rows of pitch 160 -- columns 150, 151 hold values that would win, 152 .. 160 stay poison and untouched"""
    H, W = 37, 53
    kp = ops.pad8(k)
    g = torch.Generator().manual_seed(k)
    vals = torch.randn(N, H, W, k, generator=g)
    vals[0, 0, :, :] = vals[0, 0, :, :1]                        # a row of pixels whose classes all tie: class 0
    wide = ARENA.wide(N * H * W, pitch)
    ARENA.cols(wide, 0, kp)
    acc = wide.view(N, H, W, pitch)[..., :kp]
    acc[..., :k] = vals.cuda()
    acc[..., k:] = 1e30
    pred, out = e(N, H, W, dtype=U8), e(N, k, H, W)
    ops.seg_argmax_areas(acc, k, pred=pred, seg_logits=out)
    assert torch.equal(pred.cpu().long(), vals.argmax(dim=3)) and int(pred[0, 0].max()) == 0
    assert torch.equal(out.cpu(), vals.permute(0, 3, 1, 2))
    ARENA.check()


# ------------------------------------------------------------------------------------------------ areas
@pytest.mark.parametrize("k", [2, 7, 37, 150])
@pytest.mark.parametrize("label_dtype", [U8, I64], ids=["u8", "i64"])
def test_areas_equal_the_reference_formulas(k, label_dtype):
    from mtp_amd import IoUMetric
    H, W = 37, 53
    g = torch.Generator().manual_seed(100 * k + (label_dtype == U8))
    vals = torch.randn(N, H, W, k, generator=g)
    lab = torch.randint(0, k, (N, H, W), generator=g)
    lab = torch.where(torch.rand(N, H, W, generator=g) < 0.5, vals.argmax(dim=3), lab)      # half the pixels right
    lab[torch.rand(N, H, W, generator=g) < 0.2] = 255
    pred_ref = vals.argmax(dim=3)
    ref = areas_of(pred_ref, lab, k)
    assert int(ref[0].sum()) > 0 and int(ref[2].sum()) < N * H * W
    a = torch.zeros(N, H, W, ops.pad8(k))
    a[..., :k] = vals
    acc, labd = ARENA.frozen(ARENA.like(a)), ARENA.frozen(ARENA.like(lab, dtype=label_dtype))
    # fused: arg-max + areas in one launch; two calls accumulate
    m = IoUMetric(k, iou_metrics=["mIoU", "mDice", "mFscore"])
    pred = e(N, H, W, dtype=U8)
    m.process_logits(acc, labd, pred=pred)
    assert torch.equal(pred.cpu().long(), pred_ref) and torch.equal(m.areas.cpu(), ref)
    m.process_logits(acc, labd)
    assert torch.equal(m.areas.cpu(), 2 * ref)
    # an existing prediction (uint8 and int64), onto counters preset to 2^40: the 64-bit path
    for pd in (U8, I64):
        m2 = IoUMetric(k)
        m2.areas = torch.full((3, k), 1 << 40, device="cuda", dtype=I64)
        m2.process(ARENA.frozen(ARENA.like(pred_ref, dtype=pd)), labd)
        assert torch.equal(m2.areas.cpu(), ref + (1 << 40))
    # the same input twice: identical (integer sums do not depend on the order)
    m3 = IoUMetric(k)
    m3.process_logits(acc, labd)
    assert torch.equal(m3.areas.cpu(), ref)
    # the metrics of the doubled counters = the reference formulas on them
    out = m.compute_metrics()
    tm = R.torch_metrics(2 * ref[0], 2 * (ref[1] + ref[2] - ref[0]), 2 * ref[1], 2 * ref[2], ("mIoU", "mDice", "mFscore"))
    for name, v in tm.items():
        want = (v[~v.isnan()].mean() * 100).item() if v.dim() else v.item() * 100
        assert abs(out[name if name == "aAcc" else "m" + name] - want) <= 0.005 + 1e-9, name
    m.reset()
    assert m.areas is None


def test_all_ignored_map_leaves_the_counters_zero_and_bad_labels_are_refused():
    from mtp_amd import IoUMetric
    H, W = 37, 53
    acc = ARENA.frozen(ARENA.like(torch.randn(N, H, W, 8, generator=torch.Generator().manual_seed(1))))
    m = IoUMetric(7)
    m.process_logits(acc, ARENA.frozen(ARENA.like(torch.full((N, H, W), 255), dtype=U8)))
    m.process(ARENA.like(torch.zeros(N, H, W), dtype=U8), ARENA.like(torch.full((N, H, W), 255), dtype=I64))
    assert int(m.areas.abs().sum()) == 0
    out = m.compute_metrics()
    assert all(v != v for v in out.values())                    # 0 / 0 everywhere, as the reference
    lab = torch.zeros(N, H, W, dtype=I64)
    lab[1, 2, 3] = 7
    with pytest.raises(ValueError):
        m.process_logits(acc, lab.cuda())
    lab[1, 2, 3] = -1
    with pytest.raises(ValueError):
        m.process(torch.zeros(N, H, W, dtype=U8, device="cuda"), lab.cuda())
    with pytest.raises(ValueError):
        m.process(torch.full((N, H, W), 7, dtype=U8, device="cuda"), torch.zeros(N, H, W, dtype=U8, device="cuda"))
    assert int(m.areas.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ real-valued logits
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_real_valued_logits_against_the_float64_restatement(dtype):
    """Gaussian unit-scale logits.  The bound on seg_logits: each value is a sum of at most 6 windows of 4-term interpolations in f32, a few dozen
    roundings of values of order 1, so 1e-5 * max |logit| is ample.  Measured on an MI355X: 0.08 % (f32) / 0.04 % (bf16) of pixels under the gap, max
    |seg_logits - f64| 3.1e-7 / 6.0e-8."""
    from mtp_amd import IoUMetric
    g = torch.Generator().manual_seed(3)
    wins, _ = R.slide_windows(*IMG, CROP, STRIDE)
    low = [torch.randn(N, K, CROP[0] // 4, CROP[1] // 4, generator=g) for _ in wins]
    if dtype == BF16:
        low = [x.bfloat16().float() for x in low]               # the kernel reads these very values; its arithmetic stays f32
    seg_ref = R.torch_slide_from_lowres([x.double() for x in low], CROP, STRIDE, *IMG)[0]
    sure, frac = sure_pixels(seg_ref)
    lab = torch.randint(0, K, (N, *IMG), generator=g)
    lab[torch.rand(N, *IMG, generator=g) < 0.15] = 255
    acc = accumulate(low, dtype)
    cy, cx = counts(*IMG, CROP, STRIDE)
    m = IoUMetric(K)
    pred, out = e(N, *IMG, dtype=U8), e(N, K, *IMG)
    m.process_logits(acc, ARENA.frozen(ARENA.like(lab, dtype=U8)), cy, cx, pred=pred, seg_logits=out)
    err = (out.cpu().double() - seg_ref).abs().max().item()
    print("real-valued %s: %.4f %% of pixels under the gap, max |seg_logits - f64| = %.3g" % (dtype, 100 * frac, err))
    assert err < 1e-5 * max(1.0, seg_ref.abs().max().item())
    p = pred.cpu().long()
    assert torch.equal(p[sure], seg_ref.argmax(dim=1)[sure])
    # areas: exactly those of the prediction written, hence the reference's up to the excluded pixels
    ours, ref = m.areas.cpu(), areas_of(seg_ref.argmax(dim=1), lab, K)
    assert torch.equal(ours, areas_of(p, lab, K)) and torch.equal(ours[2], ref[2])
    n_unsure = int((~sure & (lab != 255)).sum())
    assert int((ours[1] - ref[1]).abs().sum()) <= 2 * n_unsure and int((ours[0] - ref[0]).abs().sum()) <= n_unsure


# ------------------------------------------------------------------------------------------------ end to end
def _model(img_size, test_cfg, head=None):
    import mtp_amd
    torch.manual_seed(11)
    bb = mtp_amd.ViT_Win_RVSA_V3_WSZ7(img_size=img_size, patch_size=8, drop_path_rate=0.0, out_indices=[0, 1, 2, 3], embed_dim=128, depth=4, num_heads=2,
                                      mlp_ratio=4, qkv_bias=True, use_abs_pos_emb=True, interval=2, use_rel_pos_bias=True, precision="fp32",
                                      feature_dtype=torch.float32)
    Hp, Wp = bb.patch_embed.patch_shape
    if Wp > Hp:
        # the rel-pos tables of the full-attention blocks are sized from patch_shape[0] for both axes (VIT:81-84): a grid wider than tall needs a longer
        # rel_pos_w, resized as the engine's error message says (the backbone only produces features here; the new code under test starts after it)
        for blk in bb.blocks:
            if hasattr(blk.attn, "full_attn_rel_pos_w"):
                blk.attn.full_attn_rel_pos_w = torch.nn.Parameter(0.02 * torch.randn(2 * Wp - 1, blk.attn.full_attn_rel_pos_w.shape[1]))
    if head is None:
        from test_uper_head import randomise_bn
        head = randomise_bn(mtp_amd.UPerHead(in_channels=[128] * 4, channels=8, num_classes=5), 12)
        with torch.no_grad():                                    # the default N(0, 0.01) classifier puts every top-2 gap under any margin
            head.conv_seg.weight.normal_(0.0, 1.0, generator=torch.Generator().manual_seed(13))
    return mtp_amd.EncoderDecoder(bb, head, test_cfg=test_cfg).cuda()


def _record(model):
    """wrap encode_decode: keep every call's low-resolution logits (N, K, h, w) f64 on the host"""
    rec, orig, k = [], model.encode_decode, model.out_channels

    def wrapped(x):
        logits, (n, h, w) = orig(x)
        assert logits.shape == (n * h * w, ops.pad8(k)) and logits.dtype == F32 and logits[:, k:].abs().max().item() == 0.0
        rec.append(logits[:, :k].reshape(n, h, w, k).permute(0, 3, 1, 2).double().cpu())
        return logits, (n, h, w)
    model.encode_decode = wrapped
    return rec


def _check_pred(pred, seg_ref, what):
    sure, frac = sure_pixels(seg_ref)
    print("%s: %.4f %% of pixels under the gap" % (what, 100 * frac))
    assert pred.dtype == U8 and tuple(pred.shape) == (seg_ref.shape[0], *seg_ref.shape[2:])
    assert torch.equal(pred.cpu().long()[sure], seg_ref.argmax(dim=1)[sure]), what
    return sure


def test_encoder_decoder_slide_mode_with_metric_end_to_end():
    import mtp_amd
    H, W, crop, stride = 96, 128, (64, 64), (32, 48)
    m = _model(64, dict(mode="slide", crop_size=crop, stride=stride))
    g = torch.Generator().manual_seed(21)
    img = torch.randn(1, 3, H, W, generator=g).cuda()
    lab = torch.randint(0, 5, (1, H, W), generator=g)
    lab[torch.rand(1, H, W, generator=g) < 0.15] = 255
    rec = _record(m)
    metric = mtp_amd.IoUMetric(5)
    m.train()
    pred, seg = m.predict(img, return_logits=True, metric=metric, labels=lab.cuda().to(U8))
    assert m.training and m.decode_head.training and m.backbone.training          # the previous mode is restored
    assert len(rec) == 6 and tuple(rec[0].shape) == (1, 5, 16, 16)
    seg_ref = R.torch_slide_from_lowres(rec, crop, stride, H, W)[0]
    sure = _check_pred(pred, seg_ref, "slide")
    assert rel_err(seg.cpu(), seg_ref) < 1e-5
    ours, ref = metric.areas.cpu(), areas_of(seg_ref.argmax(dim=1), lab, 5)
    assert torch.equal(ours, areas_of(pred.cpu(), lab, 5)) and torch.equal(ours[2], ref[2])
    assert int((ours[1] - ref[1]).abs().sum()) <= 2 * int((~sure & (lab != 255)).sum())
    assert 0.0 < metric.compute_metrics()["mIoU"] <= 100.0
    # slide mode, padding cut off and the averaged logits resized to ori_shape before the arg-max (postprocess_result's order)
    del rec[:]
    m.eval()
    pred2 = m.predict(img, ori_shape=(90, 120), padding=(0, 4, 0, 2))
    assert not m.training
    ref2 = F.interpolate(R.torch_slide_from_lowres(rec, crop, stride, H, W)[0][:, :, :H - 2, :W - 4], size=(90, 120), mode="bilinear", align_corners=False)
    _check_pred(pred2, ref2, "slide + ori_shape")


def test_encoder_decoder_whole_mode_with_padding_and_ori_shape():
    H, W = 96, 128
    m = _model((H, W), dict(mode="whole")).eval()
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(22)).cuda()
    rec = _record(m)
    pred, seg = m.predict(img, ori_shape=(90, 120), padding=(0, 4, 0, 2), return_logits=True)
    assert len(rec) == 1 and tuple(rec[0].shape) == (1, 5, 24, 32)
    up = F.interpolate(rec[0], size=(H, W), mode="bilinear", align_corners=False)
    ref = F.interpolate(up[:, :, :H - 2, :W - 4], size=(90, 120), mode="bilinear", align_corners=False)
    _check_pred(pred, ref, "whole + ori_shape")
    assert rel_err(seg.cpu(), ref) < 1e-5
    # no padding, no ori_shape: the plain whole-image prediction
    del rec[:]
    plain = m.predict(img)
    _check_pred(plain, F.interpolate(rec[0], size=(H, W), mode="bilinear", align_corners=False), "whole")
