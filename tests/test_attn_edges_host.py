"""CPU: what tests/test_hip_attn_edges.py takes for granted about its own inputs and bounds, asserted on the very inputs of the GPU tests:
the float64 oracle is finite in every regime, the regimes are what their names say, no sample sits on a bilinear kink, a float32 evaluation of the
oracle (f32 cases) and a bf16 emulation of both attentions (P, dS and the outputs rounded to bf16; bf16 cases) stay within the room the GPU file's
bounds leave -- a QUARTER of the bound wherever EXCEPTIONS sets it (that is how those entries are made) and for all of f32; HALF of the project's table
value elsewhere in bf16, where the rounding of a bf16 output alone (2^-9 of the largest element, a third of 1.5e-2) already exceeds a quarter: a pair
beyond half would have to be listed in EXCEPTIONS -- and the two dispatch queries name, for every grid of the GPU file, the family that file asserts.
"""
import pytest
import torch

import test_hip_attn_edges as A
from oracle import vit_rvsa_oracle as O

F32, BF16 = A.F32, A.BF16
FULL, RVSA = A.full_cases(), A.rvsa_cases()


def _finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values())


def full_logits(c):
    """(B, heads, N, N) float64, the formula of oracle.full_attn_fwd"""
    B, Hp, Wp, heads, N = (c[n] for n in ("B", "Hp", "Wp", "heads", "N"))
    q, k, _ = c["qkv"].double().reshape(B, N, 3, heads, A.HD).permute(2, 0, 3, 1, 4)
    qs = q * A.SCALE
    Rh, Rw = c["rh"].double()[O._rel_index(Hp, Hp, "cpu")], c["rw"].double()[O._rel_index(Wp, Wp, "cpu")]
    q5 = qs.reshape(B, heads, Hp, Wp, A.HD)
    relh, relw = torch.einsum("byhwc,hkc->byhwk", q5, Rh), torch.einsum("byhwc,wkc->byhwk", q5, Rw)
    return ((qs @ k.transpose(-1, -2)).reshape(B, heads, Hp, Wp, Hp, Wp) + relh[..., :, None] + relw[..., None, :]).reshape(B, heads, N, N)


def bf(t):
    return t.to(BF16).to(t.dtype)


def emulate_full_bf16(c):
    """oracle.full_attn_fwd / full_attn_bwd in float64 with the roundings of a bf16 MFMA kernel: P and dS are rounded to bf16 before the P V, P^T dO,
    dS K and dS^T Q products (and the table sums), o is rounded to bf16 before it enters delta, every bf16 output is rounded"""
    B, Hp, Wp, heads, N, C = (c[n] for n in ("B", "Hp", "Wp", "heads", "N", "C"))
    hd = A.HD
    q, k, v = c["qkv"].double().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    qs = q * A.SCALE
    ih, iw = O._rel_index(Hp, Hp, "cpu"), O._rel_index(Wp, Wp, "cpu")
    Rh, Rw = c["rh"].double()[ih], c["rw"].double()[iw]
    q5 = qs.reshape(B, heads, Hp, Wp, hd)
    logits = full_logits(c)
    lse = torch.logsumexp(logits, -1)
    p = torch.exp(logits - lse[..., None])
    pb = bf(p)
    o = bf(pb @ v)
    dO = c["do"].double().reshape(B, N, heads, hd).transpose(1, 2)
    dv = pb.transpose(-1, -2) @ dO
    ds = bf(p * (dO @ v.transpose(-1, -2) - (dO * o).sum(-1, keepdim=True)))
    ds6 = ds.reshape(B, heads, Hp, Wp, Hp, Wp)
    d_relh, d_relw = ds6.sum(-1), ds6.sum(-2)
    dqs = ds @ k + (torch.einsum("byhwk,hkc->byhwc", d_relh, Rh) + torch.einsum("byhwk,wkc->byhwc", d_relw, Rw)).reshape(B, heads, N, hd)
    dk = ds.transpose(-1, -2) @ qs
    drh = torch.zeros(2 * Hp - 1, hd, dtype=torch.float64).index_add_(0, ih.reshape(-1), torch.einsum("byhwk,byhwc->hkc", d_relh, q5).reshape(-1, hd))
    drw = torch.zeros(2 * Wp - 1, hd, dtype=torch.float64).index_add_(0, iw.reshape(-1), torch.einsum("byhwk,byhwc->wkc", d_relw, q5).reshape(-1, hd))
    dqkv = bf(torch.stack([dqs * A.SCALE, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * C))
    return dict(o=o.transpose(1, 2).reshape(B * N, C), lse=lse, dqkv=dqkv, drh=drh, drw=drw)


def emulate_rvsa_bf16(c):
    """oracle.rvsa_attn_fwd / rvsa_attn_bwd in float64 with the same roundings as emulate_full_bf16: P and dS to bf16 before their products (and the
    table sums), o to bf16 before delta, the bf16 outputs (o, dqkv) rounded -- and the operands that are no inputs, the gathered K / V rows and the
    two relative-position tables, rounded to bf16 (see below).  The scatter and the coordinate gradients stay in float64"""
    B, Hp, Wp, heads, C = (c[n] for n in ("B", "Hp", "Wp", "heads", "C"))
    hd, WS, scale = A.HD, 7, A.SCALE
    qkv, samp = c["qkv"].double(), c["samp"].double()
    rel_h, rel_w, table = c["rh"].double(), c["rw"].double(), c["tab"].double()
    g = O.rvsa_geometry(Hp, Wp, WS)
    nh, nw, He, We = g["nh"], g["nw"], g["He"], g["We"]
    T = B * Hp * Wp
    qm, km, vm = (O._padded_heads(qkv[:, i * C:(i + 1) * C], B, Hp, Wp, heads, g) for i in range(3))
    ix, iy = O.rvsa_sample_coords(samp, B, Hp, Wp, heads)
    # the gathered rows are bilinear blends, not inputs: as MFMA operands they exist in bf16 only (q, k, v themselves are exact in bf16) -- with
    # logits of +-50 (R1 - R3) their 2^-9 rounding alone moves a logit by 0.1, a probability by 10 %
    ks = bf(O._bilinear_gather(km, ix, iy).reshape(B, heads, nh, nw, 49, hd))
    vs = bf(O._bilinear_gather(vm, ix, iy).reshape(B, heads, nh, nw, 49, hd))
    qw = qm.reshape(B, heads, nh, WS, nw, WS, hd).permute(0, 1, 2, 4, 3, 5, 6)
    qf = qw.reshape(B, heads, nh, nw, 49, hd)
    i7 = O._rel_index(WS, WS, "cpu")
    # the relative-position tables are MFMA operands as well (f32 parameters packed to bf16 fragments): q . R is taken with the UNSCALED q here, so in
    # R1 - R3 (|q . R| ~ 7) their rounding moves a logit by another 0.01 - 0.03
    Rh, Rw = bf(rel_h)[i7], bf(rel_w)[i7]
    relh, relw = torch.einsum("bhijxyc,xkc->bhijxyk", qw, Rh), torch.einsum("bhijxyc,ykc->bhijxyk", qw, Rw)
    a = torch.arange(WS)
    an, bn = a.repeat_interleave(WS), a.repeat(WS)
    idx = (an[:, None] - an[None, :] + WS - 1) * (2 * WS - 1) + (bn[:, None] - bn[None, :] + WS - 1)
    logits = ((qf @ ks.transpose(-1, -2)) * scale).reshape(B, heads, nh, nw, WS, WS, WS, WS) + relh[..., :, None] + relw[..., None, :]
    logits = logits.reshape(B, heads, nh, nw, 49, 49) + table[idx].permute(2, 0, 1)[None, :, None, None]
    lse = torch.logsumexp(logits, -1)
    p = torch.exp(logits - lse[..., None])
    pb = bf(p)

    def from_map(mp):
        return mp[:, :, g["pad_top"]:g["pad_top"] + Hp, g["pad_left"]:g["pad_left"] + Wp].permute(0, 2, 3, 1, 4).reshape(T, C)

    def to_map(w):   # (B,heads,nh,nw,49,hd) -> padded (B,heads,He,We,hd)
        return w.reshape(B, heads, nh, nw, WS, WS, hd).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, heads, He, We, hd)

    def to_win(t):
        return O._padded_heads(t, B, Hp, Wp, heads, g).reshape(B, heads, nh, WS, nw, WS, hd).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, heads, nh, nw, 49, hd)
    o = bf(from_map(to_map(pb @ vs)))
    dO, Ow = to_win(c["do"].double()), to_win(o)
    dvs = pb.transpose(-1, -2) @ dO
    ds = bf(p * (dO @ vs.transpose(-1, -2) - (dO * Ow).sum(-1, keepdim=True)))
    ds8 = ds.reshape(B, heads, nh, nw, WS, WS, WS, WS)
    d_relh, d_relw = ds8.sum(-1), ds8.sum(-2)
    dq = (ds @ ks) * scale + (torch.einsum("bhijxyk,xkc->bhijxyc", d_relh, Rh) + torch.einsum("bhijxyk,ykc->bhijxyc", d_relw, Rw)).reshape(B, heads, nh, nw, 49, hd)
    dks = (ds.transpose(-1, -2) @ qf) * scale
    drh = torch.zeros_like(rel_h).index_add_(0, i7.reshape(-1), torch.einsum("bhijxyk,bhijxyc->xkc", d_relh, qw).reshape(-1, hd))
    drw = torch.zeros_like(rel_w).index_add_(0, i7.reshape(-1), torch.einsum("bhijxyk,bhijxyc->ykc", d_relw, qw).reshape(-1, hd))
    dtab = torch.zeros_like(table).index_add_(0, idx.reshape(-1), ds.sum(dim=(0, 2, 3)).permute(1, 2, 0).reshape(49 * 49, heads))
    # the scatter through the bilinear weights and the coordinate gradients: autograd of the gather, fed with the emulated dK_sel / dV_sel
    kmr, vmr, spr = km.clone().requires_grad_(True), vm.clone().requires_grad_(True), samp.clone().requires_grad_(True)
    ixr, iyr = O.rvsa_sample_coords(spr, B, Hp, Wp, heads)
    ksr = O._bilinear_gather(kmr, ixr, iyr).reshape(B, heads, nh, nw, 49, hd)
    vsr = O._bilinear_gather(vmr, ixr, iyr).reshape(B, heads, nh, nw, 49, hd)
    gk, gv, gs = torch.autograd.grad((ksr * dks).sum() + (vsr * dvs).sum(), (kmr, vmr, spr), allow_unused=True)
    gs = torch.zeros_like(samp) if gs is None else gs
    dqkv = bf(torch.cat([from_map(to_map(dq)), from_map(gk), from_map(gv)], 1))
    return dict(o=o, lse=lse.reshape(B, heads, -1), dqkv=dqkv, dsamp=gs, drh=drh, drw=drw, dtab=dtab)


@pytest.mark.parametrize("case", FULL, ids=A._id)
def test_full_attention_case_is_what_the_gpu_test_assumes(case):
    key = case[:6]
    dtype, Hp, Wp, B, heads, regime = key
    c, ref = A.full_case(*key), A.full_ref(*key)
    assert _finite(ref)
    assert torch.equal(c["qkv"], c["qkv"].to(dtype).float()) and torch.equal(c["do"], c["do"].to(dtype).float())      # exact in the op's dtype
    mx, arg = full_logits(c).max(-1)                                  # (B, heads, N)
    if regime == "R2":
        # the mirror image of R3 below: one key's logit is -45.8 +- 6.9; every logit stays 5 deviations below zero and the typical row's maximum
        # (its LEAST negative logit, of up to 272) below -20, the issue's figure -- no positive or zero logit anywhere for a padding slot to hide behind
        assert float(mx.max()) < -10.0 and float(mx.median()) < -20.0 and float(ref["lse"].max()) < -10.0 + 6.0      # (lse <= max + log N, N <= 272)
    if regime == "R3":
        # one key's logit is 9/8 sum |q_d| |k_d| over 64 channels: mean 45.8, deviation 6.9 for normal q, k.  Every row stays 5 deviations above zero;
        # with >= 256 keys the typical row's maximum lies beyond +60, the issue's figure (not every row: a row's logits scale with its own |q|)
        assert float(mx.min()) > 10.0
        if c["N"] >= 256:
            assert float(mx.median()) > 60.0
    if regime == "R1":
        assert len(c["peaks"]) == (2 if B > 1 else 1)
        for b, rows, key_ in c["peaks"]:
            assert key_ == (c["N"] - 1 if b == 0 else 0)
            if c["N"] > 1:
                assert bool((arg[b][:, list(rows)] == key_).all()), "planted maximum is not the row maximum"
    # measured precision of the formula itself, against a quarter of the GPU test's bounds
    got = A.full_eval(c, torch.float32) if dtype == F32 else emulate_full_bf16(c)
    for name, (err, what) in A.errors(c, ref, {k_: v_.double() for k_, v_ in got.items()}, False).items():
        b = A.bound("full", dtype, regime, name, what)
        room = b / 4 if (dtype == F32 or ("full", A.DN[dtype], regime, name) in A.EXCEPTIONS) else b / 2
        print("host full %s %s: measured %.3g, GPU bound %.3g" % (A._id(case), name, err, b))
        assert err <= room, "%s: measured %.3g exceeds %.3g, its share of the GPU bound %.3g" % (name, err, room, b)


def test_exceptions_table_is_four_times_its_measured_values():
    for key, (measured, b) in A.EXCEPTIONS.items():
        dt = F32 if key[1] == "f32" else BF16
        table = A.TOL_LSE[dt] if key[3] == "lse" else (A.TOL[dt] if key[3] in ("o", "dq", "dk", "dv") else 10 * A.TOL[dt])
        assert b == pytest.approx(4 * measured) and measured > table / 2, key


def rvsa_measured(case):
    """{output: (error of the float32 oracle resp. the bf16 emulation against the float64 oracle, kind)}, compared as the GPU test compares"""
    key = case[:6]
    dtype, Hp, Wp, B, heads, regime = key
    c, ref = A.rvsa_case(*key), A.rvsa_ref(*key)
    got = A.rvsa_eval(c, torch.float32) if dtype == F32 else emulate_rvsa_bf16(c)
    got = {k_: v_.double() for k_, v_ in got.items()}
    errs = A.errors(c, ref, got, True)
    if regime == "R5":
        return {n: errs[n] for n in ("lse", "dq", "drh", "drw", "dtab")}
    ok = A.kink_distance(c["samp"], B, Hp, Wp, heads) >= A.KINK
    errs["dsamp"] = (A.rel_err(got["dsamp"][ok], ref["dsamp"][ok]), "tab")
    return errs


@pytest.mark.parametrize("case", RVSA, ids=A._id)
def test_rvsa_case_is_what_the_gpu_test_assumes(case):
    key = case[:6]
    dtype, Hp, Wp, B, heads, regime = key
    c, ref = A.rvsa_case(*key), A.rvsa_ref(*key)
    assert _finite(ref)
    assert torch.equal(c["qkv"], c["qkv"].to(dtype).float())
    dist = A.kink_distance(c["samp"], B, Hp, Wp, heads)
    ix, iy = A.sample_coords(c["samp"], B, Hp, Wp, heads)
    He, We = 7 * c["nh"], 7 * c["nw"]
    outside = (ix <= -1) | (ix >= We) | (iy <= -1) | (iy >= He)
    if regime == "R5":
        assert bool(outside.all())                                   # (no neighbour inside the map: no kink to sit on)
        assert float(ref["o"].abs().max()) == 0.0 and float(ref["dsamp"].abs().max()) == 0.0 and float(ref["dqkv"][:, c["C"]:].abs().max()) == 0.0
    elif regime == "R5m":
        assert float((dist >= A.KINK).double().mean()) >= 0.9
        print("host rvsa %s: %.0f %% of the samples outside the map" % (A._id(case), 100 * float(outside.double().mean())))
    else:
        assert float(dist.min()) >= A.KINK                           # no sample excluded: dsamp is compared in full
    for name, (err, what) in rvsa_measured(case).items():
        b = A.bound("rvsa", dtype, regime, name, what)
        room = b / 4 if (dtype == F32 or ("rvsa", A.DN[dtype], regime, name) in A.EXCEPTIONS) else b / 2
        print("host rvsa %s %s: measured %.3g, GPU bound %.3g" % (A._id(case), name, err, b))
        assert err <= room, "%s: measured %.3g exceeds %.3g, its share of the GPU bound %.3g" % (name, err, room, b)


def test_dispatch_queries_name_the_families_the_gpu_tests_assert():
    """the library loads without a device (as in test_abi.py): both queries swept over every grid; each family the GPU file asserts is returned for the
    grid it names, and every family the tables name is reached by some grid of the sweep"""
    from mtp_amd import ops
    ops.lib()
    for dt, Hp, Wp, _, _, _, ff, fb in FULL:
        assert ops.full_attn_kernel(dt, Hp, Wp) == ops.FULL_FWD[ff] and ops.full_attn_kernel(dt, Hp, Wp, backward=True) == ops.FULL_BWD[fb], (dt, Hp, Wp)
    for dt, Hp, Wp, _, heads, _, ff, fb in RVSA:
        assert ops.rvsa_attn_kernel(dt, Hp, Wp, heads) == ops.RVSA_FWD[ff] and ops.rvsa_attn_kernel(dt, Hp, Wp, heads, backward=True) == ops.RVSA_BWD[fb], (dt, Hp, Wp)
    seen = {"FULL_FWD": set(), "FULL_BWD": set(), "RVSA_FWD": set(), "RVSA_BWD": set()}
    for dt in (F32, BF16):
        for Hp in range(1, 65):
            for Wp in range(1, 65):
                seen["FULL_FWD"].add(ops.full_attn_kernel(dt, Hp, Wp))
                seen["FULL_BWD"].add(ops.full_attn_kernel(dt, Hp, Wp, backward=True))
                if Hp >= 7 and Wp >= 7:
                    seen["RVSA_FWD"].add(ops.rvsa_attn_kernel(dt, Hp, Wp, 3))
                    seen["RVSA_BWD"].add(ops.rvsa_attn_kernel(dt, Hp, Wp, 3, backward=True))
    tested = {"FULL_FWD": {ops.FULL_FWD[c[6]] for c in FULL}, "FULL_BWD": {ops.FULL_BWD[c[7]] for c in FULL},
              "RVSA_FWD": {ops.RVSA_FWD[c[6]] for c in RVSA}, "RVSA_BWD": {ops.RVSA_BWD[c[7]] for c in RVSA}}
    for table in seen:
        names = getattr(ops, table)
        unreached = sorted(n for n, v in names.items() if v not in seen[table])
        print("%s: no grid of 1..64 x 1..64 reaches %s" % (table, unreached or "nothing"))
        assert unreached == [], "%s names families that no grid can run: %s" % (table, unreached)
        assert seen[table] - {0} <= tested[table], "a reachable family has no case in test_hip_attn_edges.py: %s" % (seen[table] - {0} - tested[table])
