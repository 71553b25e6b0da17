"""GPU: the scene-classification kernels of csrc/cls_head.hip (mtp_gap_fwd / _bwd, mtp_cls_ce, mtp_cls_head_bwd, mtp_cls_hits), every buffer out of a
guard.Arena (poisoned outputs, guards on both sides, frozen inputs, the wrappers' own allocations included).  The reference is torch in float64 on the
same bf16-representable inputs.
  * pooling: the smallest shape, rows aligned to nothing beyond 2 bytes, both lane groupings (16 lanes per row up to 512 bytes, a wave per row beyond),
    rows longer than one pass of a wave, a row count that divides nothing, a base pointer that is only element-aligned; forward 1e-5, backward 1e-5
    (f32) or one bf16 ulp per element;
  * linear + cross-entropy: (N, C, K) from (1, 1, 1) to (64, 1536, 45) and K = 1000, both dot-product paths (C % 4 == 0 or not); loss 1e-5 relative
    and dlogits 1e-4 (the bounds seg_ce is held to), logits and prob 1e-5, pred exact under the gap condition (asserted for every sample:
    |p_a - p_j| > 1e-4 max(p_a, p_j) around the label and around the top-1 class; the seeds are the first that satisfy it);
  * regimes: all-zero weights (loss = log K, prob = 1 / K bit for bit, pred 0, the label's rank = its index), one class ahead by 200 (the other
    probabilities exactly 0, the loss of another label ~ 200, dlogits exactly +- loss_weight / N, no NaN; hits as torch's f32 CPU softmax gives them,
    a score of exactly 0 is no hit at thr = 0), loss_weight 0.4;
  * the head's backward at the same five shapes, = and +=: bound = 4 x the error of torch's own float32 CPU evaluation against float64 (floor 1e-6),
    computed here, both numbers recorded;
  * two calls of every op give the same bits;
  * hits: three batches accumulated into one counter vector, thr 0.0 and None, exact against the rank rule on the host; a constructed tie."""
import math

import pytest
import torch
import torch.nn.functional as F

import guard
from conftest import record_parity, rel_err
from mtp_amd import ops

pytestmark = pytest.mark.gpu
F32, BF16, I64, F64 = torch.float32, torch.bfloat16, torch.int64, torch.float64
GAP = 1e-4

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


def dev(t, dtype=None):
    """an op INPUT on the device, frozen"""
    return ARENA.frozen(ARENA.like(t, dtype=dtype or t.dtype))


def bf(t):
    """rounded to bf16-representable values, as f32"""
    return t.to(BF16).to(F32)


# ------------------------------------------------------------------------------------------------------------------- pooling
GAP_CASES = [(1, 1, 1, F32), (2, 5, 49, BF16), (3, 64, 196, BF16), (2, 130, 1024, F32), (2, 1536, 49, BF16), (65, 3, 4, F32),
             (2, 3, 1025, BF16),      # odd rows of the wave-per-row form, more than one pass
             (3, 7, 129, F32),        # the first f32 row length of the wave-per-row form
             (3, 7, 256, BF16)]       # the last bf16 row length of the 16-lane form


def _gap_inputs(N, C, HW, seed):
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randn(N, C, HW, generator=g)), bf(torch.randn(N, C, generator=g))


def _check_gap(x, dp, xd, dtype, tag):
    N, C, HW = x.shape
    pooled = ops.gap_fwd(xd, e(N, C))
    err = rel_err(pooled.cpu(), x.double().mean(2))
    record_parity("cls_ops", "gap_fwd_%s" % tag, err)
    assert err < 1e-5, (tag, err)
    dx = ops.gap_bwd(dev(dp), e(N, C, HW, dtype=dtype))
    ref = (dp.double() / HW).unsqueeze(2).expand(N, C, HW)
    if dtype == F32:
        err = rel_err(dx.cpu(), ref)
        assert err < 1e-5, (tag, err)
    else:
        err = float(((dx.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max())
        assert bool(((dx.cpu().double() - ref).abs() <= 2.0 ** -8 * ref.abs()).all()), (tag, err)      # one bf16 ulp, every element
    record_parity("cls_ops", "gap_bwd_%s" % tag, err)


@pytest.mark.parametrize("N,C,HW,dtype", GAP_CASES)
def test_gap_fwd_bwd_vs_float64(N, C, HW, dtype):
    x, dp = _gap_inputs(N, C, HW, 7)
    _check_gap(x, dp, dev(x, dtype), dtype, "%dx%dx%d_%s" % (N, C, HW, "bf16" if dtype == BF16 else "f32"))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_gap_fwd_base_pointer_aligned_to_one_element_only(dtype):
    N, C, HW = 2, 5, 49
    x, dp = _gap_inputs(N, C, HW, 8)
    buf = dev(torch.cat([torch.zeros(1), x.flatten()]), dtype)
    xd = buf[1:].view(N, C, HW)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == xd.element_size()
    err = rel_err(ops.gap_fwd(xd, e(N, C)).cpu(), x.double().mean(2))
    assert err < 1e-5, err


def test_gap_fixture_case(golden):
    g = golden("f20_cls_head.npz")
    x, dp = torch.from_numpy(g["b_gap_x"]).float(), torch.from_numpy(g["b_gap_dpooled"]).float()
    assert torch.equal(bf(x), x) and torch.equal(bf(dp), dp)
    pooled = ops.gap_fwd(dev(x, BF16), e(2, 5))
    assert rel_err(pooled.cpu(), g["b_gap_pooled"]) < 1e-5
    dx = ops.gap_bwd(dev(dp), e(2, 5, 49, dtype=BF16)).cpu().double()
    ref = torch.from_numpy(g["b_gap_dx"])
    assert bool(((dx - ref).abs() <= 2.0 ** -8 * ref.abs()).all())


# ------------------------------------------------------------------------------------------------------- linear + cross-entropy
CE_CASES = [(1, 1, 1), (2, 128, 7), (5, 1024, 10), (64, 1536, 45), (3, 70, 1000)]
CE_SEEDS = {(1, 1, 1): 0, (2, 128, 7): 0, (5, 1024, 10): 0, (64, 1536, 45): 0, (3, 70, 1000): 0}      # the first seeds that satisfy the gap condition


def ce_inputs(N, C, K, seed):
    """pooled ~ N(0, 1 / C) (logits of unit scale: every class takes part in the softmax), weights and bias N(0, 1), labels with 0 and K - 1"""
    g = torch.Generator().manual_seed(seed)
    pooled, w, b = bf(torch.randn(N, C, generator=g) / math.sqrt(C)), bf(torch.randn(K, C, generator=g)), bf(torch.randn(K, generator=g))
    labels = torch.randint(0, K, (N,), generator=g)
    labels[0], labels[-1] = 0, K - 1
    return pooled, w, b, labels


def ce_reference(pooled, w, b, labels, lw=1.0):
    """float64: logits, prob, pred, loss_rows, loss, dlogits"""
    logits = (pooled.double() @ w.double().t() + b.double()).requires_grad_(True)
    rows = F.cross_entropy(logits, labels, reduction="none")
    loss = lw * rows.mean()
    loss.backward()
    prob = torch.softmax(logits.detach(), 1)
    return dict(logits=logits.detach(), prob=prob, pred=prob.argmax(1), loss_rows=rows.detach(), loss=loss.detach(), dlogits=logits.grad)


def gap_condition(prob, labels):
    """for every sample and every j != a: |p_a - p_j| > 1e-4 max(p_a, p_j), a = the label and a = the top-1 class"""
    for anchor in (labels, prob.argmax(1)):
        pa = prob.gather(1, anchor.view(-1, 1))
        ok = (pa - prob).abs() > GAP * torch.maximum(pa.expand_as(prob), prob)
        ok.scatter_(1, anchor.view(-1, 1), True)
        if not bool(ok.all()):
            return False
    return True


def run_ce(pooled, w, b, labels, lw=1.0):
    N, K = pooled.shape[0], w.shape[0]
    out = ops.cls_ce(dev(pooled), dev(w), dev(b), dev(labels), lw, logits=e(N, K), prob=e(N, K), pred=e(N, dtype=I64), loss_rows=e(N), loss=e(),
                     dlogits=e(N, K))
    return {k: v.cpu() for k, v in out.items()}


def check_ce(out, ref, tag):
    errs = dict(logits=rel_err(out["logits"], ref["logits"]), prob=rel_err(out["prob"], ref["prob"]), loss_rows=rel_err(out["loss_rows"], ref["loss_rows"]),
                loss=abs(float(out["loss"]) - float(ref["loss"])) / max(abs(float(ref["loss"])), 1e-30), dlogits=rel_err(out["dlogits"], ref["dlogits"]))
    for k, v in errs.items():
        record_parity("cls_ops", "cls_ce_%s_%s" % (k, tag), v)
    assert errs["loss"] < 1e-5 and errs["loss_rows"] < 1e-5 and errs["dlogits"] < 1e-4 and errs["logits"] < 1e-5 and errs["prob"] < 1e-5, (tag, errs)
    assert torch.equal(out["pred"], ref["pred"]), tag


@pytest.mark.parametrize("N,C,K", CE_CASES)
def test_cls_ce_vs_float64(N, C, K):
    pooled, w, b, labels = ce_inputs(N, C, K, CE_SEEDS[(N, C, K)])
    assert int(labels[0]) == 0 and int(labels[-1]) == K - 1
    ref = ce_reference(pooled, w, b, labels)
    assert gap_condition(ref["prob"], labels)
    out = run_ce(pooled, w, b, labels)
    check_ce(out, ref, "%dx%dx%d" % (N, C, K))
    if (N, C, K) == (1, 1, 1):      # exactly: loss 0, dlogits 0, prob 1
        assert float(out["loss"]) == 0.0 and float(out["dlogits"].abs().max()) == 0.0 and float(out["prob"]) == 1.0
    # evaluation: no labels, the same logits / prob / pred bit for bit
    ev = ops.cls_ce(dev(pooled), dev(w), dev(b), logits=e(N, K), prob=e(N, K), pred=e(N, dtype=I64))
    assert sorted(ev) == ["logits", "pred", "prob"] and all(torch.equal(ev[k].cpu(), out[k]) for k in ev)


def test_cls_ce_fixture_case_and_loss_weight(golden):
    g = golden("f20_cls_head.npz")
    pooled, w, b = (torch.from_numpy(g["b_ce_" + k]).float() for k in ("pooled", "w", "b"))
    labels = torch.from_numpy(g["b_ce_labels"])
    ref = {k: torch.from_numpy(g["b_ce_" + k]) for k in ("logits", "prob", "pred", "loss_rows", "loss", "dlogits")}
    assert gap_condition(ref["prob"], labels)
    check_ce(run_ce(pooled, w, b, labels), ref, "f20b")
    ref4 = ce_reference(pooled, w, b, labels, 0.4)
    assert abs(float(ref4["loss"]) - 0.4 * float(ref["loss"])) < 1e-12
    check_ce(run_ce(pooled, w, b, labels, 0.4), ref4, "f20b_lw0.4")


def test_cls_ce_refuses_labels_outside_the_classes():
    pooled, w, b, labels = ce_inputs(2, 8, 3, 0)
    for bad in ([0, 3], [-1, 0]):
        with pytest.raises(ValueError):
            ops.cls_ce(dev(pooled), dev(w), dev(b), dev(torch.tensor(bad)))
    with pytest.raises(ValueError):
        ops.cls_ce(dev(pooled), dev(w), dev(b), outputs=("loss",))           # a loss without labels
    with pytest.raises(ValueError):
        ops.cls_hits(dev(pooled), dev(torch.tensor([0, 9])), (1,), ARENA.zeros(2, dtype=I64))
    with pytest.raises(ValueError):
        ops.cls_hits(dev(pooled), dev(torch.tensor([0, 1])), (1, 9), ARENA.zeros(3, dtype=I64))


def _cpu_hits(scores, labels, topk, thr):
    """the rank rule on the host: rank = #{j : s_j > s_label} + #{j < label : s_j == s_label}"""
    hits = [0] * len(topk)
    for s, l in zip(scores.tolist(), labels.tolist()):
        rank = sum(1 for j, v in enumerate(s) if v > s[l] or (v == s[l] and j < l))
        for i, k in enumerate(topk):
            hits[i] += int(rank < k and (thr is None or s[l] > thr))
    return hits + [len(labels)]


def test_regime_all_zero_weights():
    N, C, K = 3, 8, 5
    pooled = ce_inputs(N, C, K, 1)[0]
    labels = torch.tensor([0, 2, 4])
    out = run_ce(pooled, torch.zeros(K, C), torch.zeros(K), labels)
    assert abs(float(out["loss"]) - math.log(K)) < 1e-5 * math.log(K) and rel_err(out["loss_rows"], torch.full((N,), math.log(K), dtype=F64)) < 1e-5
    assert torch.equal(out["prob"], torch.full((N, K), 1.0) / K) and torch.equal(out["pred"], torch.zeros(N, dtype=I64))
    assert float(out["logits"].abs().max()) == 0.0
    # all scores tie: the label's rank is its index -> hits for k = 1 .. 5 are the labels below k
    topk = (1, 2, 3, 4, 5)
    for thr in (0.0, None):
        c = ops.cls_hits(dev(out["prob"]), dev(labels), topk, ARENA.zeros(6, dtype=I64), thr)
        assert c.cpu().tolist() == [1, 1, 2, 2, 3, 3] == _cpu_hits(out["prob"], labels, topk, thr)


def test_regime_one_class_ahead_by_200_and_loss_weight():
    N, K, lw = 4, 6, 0.4
    dom, labels = torch.tensor([1, 3, 0, 5]), torch.tensor([1, 0, 0, 2])
    pooled = 200.0 * F.one_hot(dom, K).float()            # with w = I and b = 0 the logits are exactly 200 on `dom` and 0 elsewhere
    out = run_ce(pooled, torch.eye(K), torch.zeros(K), labels, lw)
    assert torch.equal(out["logits"], pooled) and torch.equal(out["pred"], dom)
    assert all(bool(torch.isfinite(v).all()) for k, v in out.items() if k != "pred")
    cpu = torch.softmax(pooled, 1)                         # torch's f32 CPU softmax: exactly one-hot
    assert torch.equal(cpu, F.one_hot(dom, K).float()) and torch.equal(out["prob"], cpu)
    other = labels != dom
    assert rel_err(out["loss_rows"][other], torch.full((int(other.sum()),), 200.0, dtype=F64)) < 1e-5
    assert float(out["loss_rows"][~other].abs().max()) == 0.0
    assert abs(float(out["loss"]) - lw * 200.0 * float(other.sum()) / N) < 1e-5 * lw * 200.0
    step = torch.tensor(lw, dtype=F32) / N                 # exactly +- loss_weight / N on the two classes, 0 elsewhere
    want = torch.zeros(N, K)
    for n in range(N):
        if bool(other[n]):
            want[n, dom[n]], want[n, labels[n]] = step, -step
    assert torch.equal(out["dlogits"], want)
    for thr in (0.0, None):                                # thr = 0: a label whose score is exactly 0 is no hit
        c = ops.cls_hits(dev(out["prob"]), dev(labels), (1, 5), ARENA.zeros(3, dtype=I64), thr)
        assert c.cpu().tolist() == _cpu_hits(cpu, labels, (1, 5), thr)
    assert _cpu_hits(cpu, labels, (1, 5), 0.0) == [2, 2, 4] and _cpu_hits(cpu, labels, (1, 5), None) == [2, 4, 4]


# ------------------------------------------------------------------------------------------------------------ head backward
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("N,C,K", CE_CASES)
def test_cls_head_bwd_vs_float64(N, C, K, accumulate):
    g = torch.Generator().manual_seed(11)
    dl, pooled, w = bf(torch.randn(N, K, generator=g) / N), bf(torch.randn(N, C, generator=g)), bf(torch.randn(K, C, generator=g))
    dw0, db0 = bf(torch.randn(K, C, generator=g)), bf(torch.randn(K, generator=g))
    if not accumulate:
        dw0, db0 = torch.zeros(K, C), torch.zeros(K)

    def evaluate(t):
        return dict(dw=dw0.to(t) + dl.to(t).t() @ pooled.to(t), db=db0.to(t) + dl.to(t).sum(0), dpooled=dl.to(t) @ w.to(t))
    ref, cpu32 = evaluate(F64), evaluate(F32)
    dw, db = (ARENA.like(dw0), ARENA.like(db0)) if accumulate else (e(K, C), e(K))
    out = dict(zip(("dw", "db", "dpooled"), ops.cls_head_bwd(dev(dl), dev(pooled), dev(w), dw, db, e(N, C), accumulate=accumulate)))
    for k in ("dw", "db", "dpooled"):
        e32 = rel_err(cpu32[k], ref[k])                    # torch's own float32 evaluation on the CPU against float64
        err = rel_err(out[k].cpu(), ref[k])
        tag = "%s_%dx%dx%d_%s" % (k, N, C, K, "acc" if accumulate else "set")
        record_parity("cls_ops", "cls_head_bwd_" + tag, err)
        record_parity("cls_ops", "cls_head_bwd_torch_f32_cpu_" + tag, e32)
        assert err < max(4 * e32, 1e-6), (tag, err, e32)
    # without dpooled: the same dw / db
    dw2, db2 = (ARENA.like(dw0), ARENA.like(db0)) if accumulate else (e(K, C), e(K))
    ops.cls_head_bwd(dev(dl), dev(pooled), dev(w), dw2, db2, None, accumulate=accumulate)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


# ------------------------------------------------------------------------------------------------------------ determinism
def test_two_calls_give_the_same_bits():
    x, dp = _gap_inputs(3, 64, 196, 3)
    xd, dpd = dev(x, BF16), dev(dp)
    assert torch.equal(ops.gap_fwd(xd, e(3, 64)), ops.gap_fwd(xd, e(3, 64)))
    assert torch.equal(ops.gap_bwd(dpd, e(3, 64, 196, dtype=BF16)), ops.gap_bwd(dpd, e(3, 64, 196, dtype=BF16)))
    x, _ = _gap_inputs(2, 130, 1024, 4)
    xd = dev(x)
    assert torch.equal(ops.gap_fwd(xd, e(2, 130)), ops.gap_fwd(xd, e(2, 130)))
    N, C, K = 64, 1536, 45
    pooled, w, b, labels = ce_inputs(N, C, K, 5)
    a, c = run_ce(pooled, w, b, labels, 0.4), run_ce(pooled, w, b, labels, 0.4)
    assert all(torch.equal(a[k], c[k]) for k in a) and len(a) == 6
    dl, pd, wd = dev(a["dlogits"]), dev(pooled), dev(w)
    r = [ops.cls_head_bwd(dl, pd, wd, e(K, C), e(K), e(N, C)) for _ in range(2)]
    assert all(torch.equal(p, q) for p, q in zip(*r))
    s, l = dev(a["prob"]), dev(labels)
    h = [ops.cls_hits(s, l, (1, 5), ARENA.zeros(3, dtype=I64)) for _ in range(2)]
    assert torch.equal(h[0], h[1])


# ------------------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("thr", [0.0, None])
def test_cls_hits_three_batches_accumulated(thr):
    g = torch.Generator().manual_seed(21)
    counters = ARENA.zeros(3, dtype=I64)
    want = [0, 0, 0]
    for n in (1, 7, 64):
        scores = torch.randn(n, 10, generator=g)          # raw scores, about half of them <= 0: the threshold decides
        labels = torch.randint(0, 10, (n,), generator=g)
        ops.cls_hits(dev(scores), dev(labels), (1, 5), counters, thr)
        want = [a + c for a, c in zip(want, _cpu_hits(scores, labels, (1, 5), thr))]
    assert counters.cpu().tolist() == want and want[2] == 72 and 0 < want[0] < want[1] < 72


def test_cls_hits_constructed_tie_and_large_k():
    scores = torch.tensor([[0.4, 0.1, 0.4, 0.1], [0.4, 0.1, 0.4, 0.1], [0.1, 0.2, 0.3, 0.4]])
    labels = torch.tensor([2, 0, 3])                      # the label at the higher index of two equal scores ranks second
    c = ops.cls_hits(dev(scores), dev(labels), (1, 2), ARENA.zeros(3, dtype=I64))
    assert c.cpu().tolist() == [2, 3, 3] == _cpu_hits(scores, labels, (1, 2), 0.0)
    g = torch.Generator().manual_seed(22)                 # K beyond one wave, eight k values, counters preset beyond 2^32
    scores, labels = torch.randn(9, 1000, generator=g), torch.randint(0, 1000, (9,), generator=g)
    topk = (1, 2, 5, 10, 100, 500, 999, 1000)
    c = ARENA.zeros(9, dtype=I64)
    c += 1 << 40
    ops.cls_hits(dev(scores), dev(labels), topk, c, None)
    assert (c.cpu() - (1 << 40)).tolist() == _cpu_hits(scores, labels, topk, None)
