"""CPU: the float64 optimizer reference and layout helpers of tests/optim_ref.py, which tests/test_hip_step_edges.py holds the HIP kernels to, against
what they restate: torch.optim.AdamW after clip_grad_norm_, ops._wimg_table's tile bookkeeping, and the exactness claim of exact_ints."""
import pytest
import torch

import optim_ref as R

F64 = torch.float64


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
def test_adamw_ref_is_torch_adamw_after_clip_grad_norm(clip, grad_scale):
    """five steps, four groups with their own lr scale and weight decay; the torch side scales its gradients by grad_scale, clips, steps.  Both sides
    in float64 from the same double hyper-parameters: they differ in the order of a few operations only (lerp, sqrt(v) / sqrt(bc2)), <= 1e-12 relative"""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    sizes, sc, wd = [64, 192, 128, 64], [1.0, 0.81, 0.5, 0.9], [0.05, 0.0, 0.1, 0.15]
    start = [0, 64, 256, 384]
    n = sum(sizes)
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(n, generator=gen, dtype=F64)
    m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    ref = [p[a:a + k].clone().requires_grad_(True) for a, k in zip(start, sizes)]
    opt = torch.optim.AdamW([{"params": [q], "lr": lr * s, "weight_decay": w} for q, s, w in zip(ref, sc, wd)], lr=lr, betas=(b1, b2), eps=eps)
    # norm of the scaled gradients ~ sqrt(448) grad_scale: 21 resp. 2.6 -- clipped by max_norm 1, far from clipped by 1e3
    max_norm = 1.0 if clip else 1e3
    for t in range(1, 6):
        g = torch.randn(n, generator=gen, dtype=F64)
        for q, a, k in zip(ref, start, sizes):
            q.grad = g[a:a + k] * grad_scale
        norm = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        assert (float(norm) > 2 * max_norm) if clip else (float(norm) < 0.5 * max_norm)
        opt.step()
        hyper = [lr, b1, b2, eps, 1 - b1 ** t, 1 - b2 ** t]
        p, m, v = R.adamw_ref(p, g, m, v, start, wd, sc, hyper, float((g * g).sum()), max_norm, grad_scale)
    got = torch.cat([q.detach() for q in ref])
    assert float(((p - got).abs() / got.abs().clamp_min(1e-30)).max()) <= 1e-12
    state = [opt.state[q] for q in ref]
    tm, tv = torch.cat([s["exp_avg"] for s in state]), torch.cat([s["exp_avg_sq"] for s in state])
    assert float(((m - tm).abs() / tm.abs().clamp_min(1e-300)).max()) <= 1e-12 and float(((v - tv).abs() / tv.abs().clamp_min(1e-300)).max()) <= 1e-12


def test_adamw_ref_without_a_norm_and_without_lr_scales():
    """sqn = None: grad_scale alone; seg_lr = None: scale 1 everywhere; f32 inputs are taken at their f32 values"""
    p, g = torch.randn(128, generator=torch.Generator().manual_seed(1)), torch.randn(128, generator=torch.Generator().manual_seed(2))
    z = torch.zeros(128)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001])
    a = R.adamw_ref(p, g, z, z, [0, 64], [0.05, 0.0], None, hyper, None, 5.0, 0.125)
    b = R.adamw_ref(p, g * 0.125, z, z, [0, 64], [0.05, 0.0], [1.0, 1.0], hyper, None, 0.0, 1.0)
    assert all(x.dtype == F64 and torch.equal(x, y) for x, y in zip(a, b))
    assert R.clip_scale(None, 5.0, 0.125) == 0.125 and R.clip_scale(4.0, 1e3, 0.5) == 0.5
    assert abs(R.clip_scale(400.0, 5.0, 0.5) - 0.5 * 5.0 / (10.0 + 1e-6)) < 1e-15
    lr32 = float(torch.tensor(1e-3))
    assert torch.equal(a[0][64:], p[64:].double() - (lr32 / float(hyper[4])) * a[1][64:] / (a[2][64:].sqrt() * float(hyper[5]) ** -0.5 + float(hyper[3])))


def test_layout_offsets_and_tiles_are_those_of_the_wimg_table():
    from mtp_amd import ops
    segs, total = R.layout(R.SEAM_SHAPES)
    assert total % 64 == 0 and all(s["off"] % 64 == 0 for s in segs)
    off = 0
    for s, (shape, _, _, _) in zip(segs, R.SEAM_SHAPES):       # FlatParams: offsets advance by the element count rounded up to 64
        assert s["off"] == off and s["numel"] == R._numel(shape)
        off += (s["numel"] + 63) // 64 * 64
    assert off == total
    rows = [(0, None, None, s["R"], s["C"], s["f32_out"], 0.0) for s in segs]
    table, tiles, _ = ops._wimg_table(rows, "cpu")
    assert tiles == R.total_tiles(segs)
    from mtp_amd import _lib
    arr = (_lib.WimgDesc * len(segs)).from_buffer_copy(bytes(table.numpy().tobytes()))
    assert [d.tile0 for d in arr] == [s["tile0"] for s in segs] and [(d.R, d.C) for d in arr] == [(s["R"], s["C"]) for s in segs]
    mine = R.wimg_descs(segs, torch.zeros(total), [None] * len(segs), [0.0] * len(segs))
    assert [(d.R, d.C, d.tile0, d.f32_out) for d in mine] == [(d.R, d.C, d.tile0, d.f32_out) for d in arr]
    assert [d.src - mine[0].src for d in mine] == [4 * s["off"] for s in segs]
    # the list covers what it says: every image combination, both image dtypes, the 1-D sizes, an element-wise pair
    assert {(s["has_w"], s["has_wt"]) for s in segs} == {(True, True), (True, False), (False, True), (False, False)}
    assert {s["f32_out"] for s in segs if s["has_w"] or s["has_wt"]} == {True, False}
    assert {s["numel"] for s in segs if len(s["shape"]) == 1} == {1, 4, 63, 64, 65} and any(s["shape"] == (10, 6) for s in segs)
    assert {d for s in segs if len(s["shape"]) == 2 for d in s["shape"]} <= {1, 4, 8, 12, 60, 64, 68, 72, 136, 10, 6}


def test_exact_ints_sums_are_exact_in_f32():
    for n in R.SQNORM_SIZES + [R.SEGMENT_BASE] + R.REDUCE_SIZES:
        x = R.exact_ints(n, seed=n % 7)
        assert x.dtype == torch.float32 and x.numel() == n and n < 2 ** 24
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert int((x * x).sum(dtype=F64)) == int((x != 0).sum()) < 2 ** 24
        if n > 100:
            assert 0.5 * n < int((x != 0).sum()) < 0.8 * n and int((x > 0).sum()) > 0.25 * n      # all three values, in earnest
    with pytest.raises(AssertionError):
        R.exact_ints(2 ** 24)
    assert not torch.equal(R.exact_ints(1024, 0), R.exact_ints(1024, 1))
