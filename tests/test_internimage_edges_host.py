"""CPU: what tests/test_hip_internimage_edges.py takes for granted about its own inputs and bounds, asserted on the very inputs of the GPU tests: every
DCNv3 regime is what its name says (through dcnv3_oracle._locations), the float64 oracle is finite, the oracle evaluated in float32 stays within a QUARTER
of the fp32 bounds in the regimes that put samples on cell edges (the one-sided derivative at an exact integer position is deterministic there), a float32
CPU evaluation of every summing operator stays within HALF of the arithmetic bound at every listed shape, and the two dispatch queries -- pure host
functions -- name, for every case of the GPU file, the family that file asserts."""
import pytest
import torch

import test_hip_internimage_edges as E
from oracle import dcnv3_oracle as D

F32, BF16 = E.F32, E.BF16
CASES = E.dcn_cases()


def locations(case):
    c = E.dcn_case(*case)
    N, H, W, G = c["grid"]
    lh, lw = D._locations(c["off"].double(), H, W, *c["args"][:8], G, c["args"][10], c["rmc"])
    return c, lh, lw


@pytest.mark.parametrize("case", CASES, ids=E.dcn_id)
def test_dcnv3_regimes_are_what_their_names_say(case):
    regime, grid, os_, GC, rmc = case
    c, lh, lw = locations(case)
    N, H, W, G = grid
    assert all(bool(torch.isfinite(v).all()) for v in c["ref"].values())
    assert torch.equal(c["x"].to(BF16).float(), c["x"]) and torch.equal(c["mask"].to(BF16).float(), c["mask"]) and torch.equal(c["gout"].to(BF16).float(), c["gout"])
    valid = (lh > -1) & (lw > -1) & (lh < H) & (lw < W)
    edge = lambda t: (t - t.round()).abs()
    if regime == "zero":
        assert float(c["off"].abs().max()) == 0.0 and float(torch.maximum(edge(lh), edge(lw)).max()) == 0.0                # every sample on a pixel centre
    elif regime == "integer":
        assert float(torch.maximum(edge(lh), edge(lw)).max()) == 0.0                           # every sample on a cell edge
        assert bool((lw == -1).any()) and bool(((lh == H) | (lw == W)).any())                  # exactly -1; exactly H or W
    elif regime in ("quarter", "one_hot_mask", "zero_mask"):
        assert float(torch.minimum(edge(lh), edge(lw)).min()) >= 0.25                          # clear of every kink
        m = c["mask"].reshape(N, H, W, G, 9 - rmc)
        if regime == "one_hot_mask":
            assert bool((m.sum(-1) == 1).all()) and bool(((m == 0) | (m == 1)).all())
        if regime == "zero_mask":
            assert float(m.abs().max()) == 0.0
    elif regime == "outside":
        assert not bool(valid.any())
        assert bool(((lh <= -2) | (lh >= H + 1) | (lw <= -2) | (lw >= W + 1)).all())           # more than one pixel outside
        assert all(float(v.abs().max()) == 0.0 for v in c["ref"].values())
    elif regime == "reach":
        # corners (floor, floor + 1 per axis) relative to the sample's own output pixel: within R = gathered, beyond = the atomic path (window form); relative
        # to the nominal position with a reach of one pixel for the 3 x 3 form.  Only a map wider than the reach can hold a valid sample at its border
        R = E.reach_of(os_)
        ho, wo = torch.arange(H).view(1, H, 1, 1, 1), torch.arange(W).view(1, 1, W, 1, 1)
        far = lambda lo, o, r: ((lo - o).abs() > r) | ((lo + 1 - o).abs() > r)
        fh, fw = torch.floor(lh), torch.floor(lw)
        beyond = (far(fh, ho, R) | far(fw, wo, R)) & valid
        if max(H, W) > R + 1:
            assert bool(beyond.any()) and bool((~beyond & valid).any())
            last = valid & (((fh + 1 - ho).abs() == R) | ((fw + 1 - wo).abs() == R) | ((fh - ho).abs() == R) | ((fw - wo).abs() == R))
            assert bool(last.any())                                                            # a corner exactly on the last position inside
        if os_ in (1.0, 2.0) and max(H, W) > 2:
            pts = D._points(3, 3, rmc)
            nh = ho + torch.tensor([(p[1] - 1) * os_ for p in pts]).view(1, 1, 1, 1, -1)
            nw = wo + torch.tensor([(p[0] - 1) * os_ for p in pts]).view(1, 1, 1, 1, -1)
            b3 = (far(fh, nh, 1) | far(fw, nw, 1)) & valid
            assert bool(b3.any()) and bool((~b3 & valid).any())


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("integer", "quarter", "reach")], ids=E.dcn_id)
def test_float32_oracle_stays_within_a_quarter_of_the_fp32_bounds(case):
    c = E.dcn_case(*case)
    y = D.dcnv3_forward(c["x"], c["off"], c["mask"], *c["args"], c["rmc"])
    gi, go, gm = D.dcnv3_backward(c["x"], c["off"], c["mask"], *c["args"], c["gout"], c["rmc"])
    for name, got in (("out", y), ("grad_input", gi), ("grad_offset", go), ("grad_mask", gm)):
        ref = c["ref"][name]
        if float(ref.abs().max()) == 0.0:
            assert float(got.abs().max()) == 0.0, name
        else:
            assert E.rel_err(got, ref) < 0.25 * E.DCN_TOL[F32][name], name


def half(bound):
    return 0.5 * bound


@pytest.mark.parametrize("shape,k", [(s, 3) for s in E.DW3_SHAPES] + [(s, k) for s in E.DWK_SHAPES for k in E.DWK_KS])
def test_float32_depthwise_convolutions_stay_within_half_the_bound(shape, k):
    c = E.dwconv_case(*shape, k)
    rows = shape[0] * shape[1] * shape[2]
    y, dx, dw, db = E.dwconv_eval(c["x"], c["dy"], c["w"], c["b"], k, F32)
    E.within(y, c["y"], half(E.sum_bound(k * k + 1, c["ymag"], c["y"])), "fwd")
    E.within(dx, c["dx"], half(E.sum_bound(k * k + 1, c["dxmag"], c["dx"])), "dx")
    E.within(dx + c["base"], c["dx"] + c["base"].double(), half(E.sum_bound(k * k + 1, c["dxmag"] + c["base"].double().abs(), c["dx"])), "dx +=")
    E.within(dw, c["dw"], half(E.sum_bound(rows, c["dwmag"], c["dw"])), "dw")
    E.within(db, c["db"], half(E.sum_bound(rows, c["dbmag"], c["db"])), "db")
    # (a bf16 output: the 2^-8 |ref| term IS the worst rounding of an 8-bit significand, half an ulp at the foot of a binade -- room only in the f32 part)
    E.within(y.to(BF16), c["y"], half(E.sum_bound(k * k + 1, c["ymag"], c["y"])) + 2.0 ** -8 * c["y"].abs(), "fwd bf16")


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,H,W,Cin,nchw", E.I2C_SHAPES)
def test_float32_col2im_stays_within_half_the_bound(N, H, W, Cin, nchw, stride, extra):
    c = E.i2c_case(N, H, W, Cin, stride, extra)
    assert c["Kp"] >= 9 * Cin and c["Kp"] % 8 == 0 and float(c["cols"][:, 9 * Cin:].abs().sum()) == 0.0
    dx = E.gather3x3_eval(c["x"], c["dcols"], stride, c["Kp"], F32)[1]
    E.within(dx, c["dx"], half(E.sum_bound(10, c["dxmag"], c["dx"])), "col2im")
    E.within(dx + c["base"], c["dx"] + c["base"].double(), half(E.sum_bound(10, c["dxmag"] + c["base"].double().abs(), c["dx"])), "col2im +=")


@pytest.mark.parametrize("rows,Cc,rps", [(1, 4, 1), (257, 4, 100), (130, 1028, 7)])
def test_float32_scale_residual_stays_within_half_the_bound(rows, Cc, rps):
    c = E.scale_residual_case(rows, Cc, rps)
    srow = c["s"].repeat_interleave(rps)[:rows, None]
    out = c["x"] + srow * c["gamma"] * c["z"]
    E.within(out, c["out"], half(E.sum_bound(3, c["outmag"], c["out"])), "out")
    E.within(srow * c["gamma"] * c["do"], c["dz"], half(E.sum_bound(3, c["dz"].abs(), c["dz"])), "dz")
    E.within((srow * c["do"] * c["z"]).sum(0), c["dg"], half(E.sum_bound(rows + 2, c["dgmag"], c["dg"])), "dgamma")
    assert bool((c["s"] == 0).any())


def test_softmax_and_gate_inputs_are_what_the_gpu_file_says():
    for regime in E.SMX_REGIMES:
        for P in (8, 9, 25):
            lg = E.softmax_logits(regime, 3, 2, P, 2 * P + 7)
            v = lg[:, :2 * P].reshape(3, 2, P)
            p = torch.softmax(v.double(), -1)
            assert bool(torch.isfinite(p).all()) and float((p.sum(-1) - 1).abs().max()) < 1e-12 and float(lg[:, 2 * P:].min()) == 100.0
            if regime == "ulp_ramp":
                d = v[..., 1:] - v[..., :-1]
                assert bool((d == 0.125).all()) and bool((v.to(BF16).float() == v).all()) and 16 <= float(v.min()) and float(v.max()) < 32
            if regime == "one_high":
                assert bool(((v == 60).sum(-1) == 1).all()) and bool(((v == 0) | (v == 60)).all())
    for sign in (1, -1, 0):
        c = E.cfs_case(5, 3, 4, 8, sign)
        assert bool((c["lpad"][:, :3].abs() == 40).all()) and all(bool(torch.isfinite(c[k]).all()) for k in ("out", "dy", "dxp", "dl"))


# ---- the dispatch queries without a device: CPU tensors of the cases' shapes stand in for the arena buffers (the allocator aligns them to 64 bytes)
@pytest.mark.parametrize("dtype", E.DT, ids=E.DTID)
def test_dcnv3_query_names_the_family_the_gpu_file_asserts(dtype, monkeypatch):
    from mtp_amd.ops_dcnv3 import functions as Fn
    for case in CASES:
        regime, grid, os_, GC, rmc = case
        c = E.dcn_case(*case)
        x, off, m, gout = (c[k].to(dtype) for k in ("x", "off", "mask", "gout"))
        grads = [torch.empty(t.shape) for t in (x, off, m)]
        assert E.aligned(x, off, m, gout, *grads)
        for variant in (0, 8):
            monkeypatch.setenv("MTP_DCNV3_VARIANT", str(variant))
            assert Fn.dcnv3_kernel(x, off, m, gout, *c["args"], 256, rmc) == Fn.DCNV3_KERNEL[E.want_fwd(GC, rmc, variant)], case
        for variant in E.VARIANTS:
            monkeypatch.setenv("MTP_DCNV3_VARIANT", str(variant))
            assert Fn.dcnv3_kernel(x, off, m, gout, *c["args"], 256, rmc, grads=grads) == Fn.DCNV3_KERNEL[E.want_bwd(GC, os_, variant)], (case, variant)
    want = {(8, 0): "fwd9", (4, 0): "fwd_scalar", (16, 1): "fwd_vec8", (16, 0): "fwd9"}
    assert all(E.want_fwd(GC, rmc, 0) == v for (GC, rmc), v in want.items()) and E.want_fwd(8, 0, 8) == "fwd_vec8"
    assert {E.want_bwd(16, s, 0) for s in (1.0, 2.0, 0.5)} == {"bwd_window_r2", "bwd_window_r3"} and E.want_bwd(16, 0.5, 4) == "bwd_window_r2"


@pytest.mark.parametrize("dtype", E.DT, ids=E.DTID)
def test_conv_query_names_the_family_the_gpu_file_asserts(dtype):
    from mtp_amd import ops
    K = ops.CONV_KERNEL
    for N, H, W, Cc in E.DW3_SHAPES:
        x, y, dx = torch.empty(N * H * W, Cc, dtype=dtype), torch.empty(N * H * W, Cc, dtype=dtype), torch.empty(N * H * W, Cc)
        w, b = torch.empty(Cc * 9 + 4), torch.empty(Cc)
        assert E.aligned(x, y, dx, w, b)
        assert ops.conv_kernel("dwconv3x3_fwd", x, y, N, H, W, Cc, w=w, b=b) == K[E.want_dw3("dwconv3x3_fwd", dtype, W)]
        assert ops.conv_kernel("dwconv3x3_bwd_dx", x, dx, N, H, W, Cc, w=w) == K[E.want_dw3("dwconv3x3_bwd_dx", dtype, W)]
        assert ops.conv_kernel("dwconv3x3_bwd_dw", x, None, N, H, W, Cc) == K[E.want_dw3("dwconv3x3_bwd_dw", dtype, W)]
        assert ops.conv_kernel("dwconv3x3_fwd", x, y, N, H, W, Cc, w=w[1:], b=b) == K["element"]      # weights 4 bytes past a 16-byte boundary
        assert (E.want_dw3("dwconv3x3_fwd", BF16, W) == "p8") == (W % 8 == 0) and (E.want_dw3("dwconv3x3_bwd_dw", BF16, W) == "px4") == (W % 4 == 0)
    lib = ops.lib()
    assert E.dw3_empty_blocks(lib, 1, 151, 28) == 0 and E.dw3_empty_blocks(lib, 1, 363, 364) >= 1
    for N, H, W, Cin, nchw in E.I2C_SHAPES:
        for stride in (1, 2):
            for extra in (0, 8):
                Ho, Wo, Kp = (H - 1) // stride + 1, (W - 1) // stride + 1, E.pad8(9 * Cin) + extra
                src = torch.empty(N * H * W * Cin, dtype=F32 if nchw else dtype)
                strides = (Cin * H * W, W, 1, H * W) if nchw else (H * W * Cin, W * Cin, Cin, 1)
                cols, dx = torch.empty(N * Ho * Wo, Kp, dtype=dtype), torch.empty(N * H * W * (Cin + 4))
                want = K[E.want_i2c(dtype, Cin, nchw)]
                assert (want == K["v8"]) == (dtype == BF16 and Cin % 8 == 0)
                assert ops.conv_kernel("im2col3x3", src, cols, N, H, W, Cin, strides, stride, Kp) == want
                assert ops.conv_kernel("col2im3x3", cols, dx, N, H, W, Cin, strides, stride, Kp) == want
                ldw = Cin + 4
                assert ops.conv_kernel("col2im3x3", cols, dx, N, H, W, Cin, (H * W * ldw, W * ldw, ldw, 1), stride, Kp) == K["element"]
