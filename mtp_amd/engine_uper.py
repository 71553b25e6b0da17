"""Explicit forward / backward schedule of the UperNet decode head (mmseg UPerHead) on libmtp_hip.so.

Every map is channels-last (rows = N*H*W, C).  Convolutions are GEMMs: 1x1 = mtp_gemm_nt on the rows, 3x3 = mtp_im2col3x3 + mtp_gemm_nt, worked in
sample chunks so the column buffer stays under COLS_BUDGET bytes; their gradients are mtp_gemm_tn (weights) and mtp_gemm_nt + mtp_col2im3x3 (data).
BatchNorm + ReLU, bilinear resize, adaptive pooling, Dropout2d and the segmentation loss are the kernels of csrc/decode_head.hip.  ACT (the GEMM
operands, the BN outputs) is f32 in 'fp32' mode and bf16 in 'bf16' mode; BN statistics, the logits and every gradient buffer are f32.

SyncBN: `reduce` (a callable that sums an f32 tensor over the ranks, in place, and returns it) is applied to each BN layer's (sum x, sum x^2, count)
between the statistics and the apply launch, and to (sum dy', sum dy' xhat) in the backward -- what torch.nn.SyncBatchNorm exchanges.
"""
import torch

from . import ops

F32 = torch.float32
COLS_BUDGET = 256 << 20      # bytes of im2col columns (or of their gradient) per chunk


class UperEngine:
    def __init__(self, head, precision="fp32"):
        self.h = head
        self.act = F32 if precision == "fp32" else torch.bfloat16

    # ------------------------------------------------------------------ plumbing
    def _e(self, *shape, dtype=None):
        return torch.empty(*shape, device=self.dev, dtype=dtype or self.act)

    def _z(self, *shape, dtype=F32):
        return torch.zeros(*shape, device=self.dev, dtype=dtype)

    def _w1(self, name, rows_pad=None):
        """1x1 conv weight (Cout, Cin, 1, 1) f32 -> (w (Rp, Cin), wT (Cin, Rp)) ACT, rows Cout .. Rp zero"""
        w = self.P[name]
        R, Cc = w.shape[0], w.shape[1]
        Rp = rows_pad or R
        wp, wpt = self._e(Rp, Cc), self._e(Cc, Rp)
        ops.pack_rows_padded(w.reshape(R, Cc), wp, wpt)
        return wp, wpt

    def _w3(self, name):
        w = self.P[name]
        Kp = ops.pad8(9 * w.shape[1])
        w2, w2t = self._e(w.shape[0], Kp), self._e(Kp, w.shape[0])
        ops.conv3x3_pack(w, w2, w2t)
        return w2, w2t

    # ------------------------------------------------------------------ BatchNorm + ReLU
    def _bn_fwd(self, z, pre, out):
        """z (rows, C) ACT conv output -> out (rows, C) ACT (a column slice is fine); returns what the backward needs"""
        P, C = self.P, z.shape[1]
        mean, rstd = self._e(C, dtype=F32), self._e(C, dtype=F32)
        b = pre + ".bn."
        if self.training:
            # two passes: a first mean, then the sums centred on it (exact variance when |mean| >> std); SyncBN all-reduces both
            count = self.count_of(z.shape[0])
            s1 = ops.bn_sums(z)
            if self.reduce is not None:
                s1 = self.reduce(s1)
            center = self._e(C, dtype=F32)
            ops.bn_finalize(s1, count, None, None, center, rstd)
            sums = ops.bn_sums(z, center)
            if self.reduce is not None:
                sums = self.reduce(sums)
            ops.bn_finalize(sums, count, P[b + "running_mean"], P[b + "running_var"], mean, rstd, momentum=0.1, eps=1e-5, center=center)
            self.P[b + "num_batches_tracked"].add_(1)
        else:
            count = 0.0
            ops.bn_finalize(None, 0.0, P[b + "running_mean"], P[b + "running_var"], mean, rstd, eps=1e-5)
        ops.bn_apply(z, mean, rstd, P[b + "weight"], P[b + "bias"], out, relu=True)
        return (z, mean, rstd, count)

    def count_of(self, rows):
        return self._counts[rows]

    def _bn_bwd(self, dy, saved, pre, G):
        """dy (rows, C) f32 -> dz (rows, C) ACT; d gamma / d beta (this rank's sums) into G"""
        z, mean, rstd, count = saved
        P, C = self.P, z.shape[1]
        b = pre + ".bn."
        sums = None
        if self.training:
            local = ops.bn_bwd_sums(dy, z, mean, rstd, P[b + "weight"], P[b + "bias"])
            G[b + "bias"].copy_(local[:C])
            G[b + "weight"].copy_(local[C:])
            sums = local if self.reduce is None else self.reduce(local.clone())
        else:
            sums_eval = ops.bn_bwd_sums(dy, z, mean, rstd, P[b + "weight"], P[b + "bias"])
            G[b + "bias"].copy_(sums_eval[:C])
            G[b + "weight"].copy_(sums_eval[C:])
        return ops.bn_bwd_dx(dy, z, mean, rstd, P[b + "weight"], P[b + "bias"], sums, count, self._e(*z.shape))

    # ------------------------------------------------------------------ ConvModules
    def _cm1_fwd(self, x, pre, out=None):
        """ConvModule 1x1: x (rows, Cin) ACT -> (rows, C) ACT"""
        wp, wpt = self._w1(pre + ".conv.weight")
        z = ops.gemm_nt(x, wp, self._e(x.shape[0], wp.shape[0]))
        out = self._e(*z.shape) if out is None else out
        return out, dict(x=x, wpt=wpt, bn=self._bn_fwd(z, pre, out))

    def _cm1_bwd(self, dy, c, pre, G, need_dx=True):
        dz = self._bn_bwd(dy, c["bn"], pre, G)
        ops.gemm_tn(dz, c["x"], G[pre + ".conv.weight"].view(dz.shape[1], -1))
        return ops.gemm_nt(dz, c["wpt"], self._e(dz.shape[0], c["wpt"].shape[0], dtype=F32)) if need_dx else None

    def _chunks(self, N, HW, Kp):
        per = max(1, COLS_BUDGET // max(1, HW * Kp * 4))
        return [(n0, min(N, n0 + per)) for n0 in range(0, N, per)]

    def _cm3_fwd(self, x, N, H, W, pre, out=None):
        """ConvModule 3x3 (padding 1): x (N*H*W, Cin) ACT (a column slice is fine) -> (rows, C) ACT"""
        w2, w2t = self._w3(pre + ".conv.weight")
        Cin, ld, HW = x.shape[1], x.stride(0), H * W
        z = self._e(x.shape[0], w2.shape[0])
        for n0, n1 in self._chunks(N, HW, w2.shape[1]):
            cols = ops.im2col3x3(x[n0 * HW:n1 * HW], (HW * ld, W * ld, ld, 1), self._e((n1 - n0) * HW, w2.shape[1]), n1 - n0, H, W, Cin, 1)
            ops.gemm_nt(cols, w2, z[n0 * HW:n1 * HW])
        out = self._e(*z.shape) if out is None else out
        return out, dict(x=x, w2t=w2t, geom=(N, H, W), bn=self._bn_fwd(z, pre, out))

    def _cm3_bwd(self, dy, c, pre, G, dx):
        """dx: (rows, Cin) f32 (a column slice is fine) = the data gradient"""
        dz = self._bn_bwd(dy, c["bn"], pre, G)
        x, w2t = c["x"], c["w2t"]
        N, H, W = c["geom"]
        Cin, ld, HW, Kp, Cout = x.shape[1], x.stride(0), H * W, w2t.shape[0], w2t.shape[1]
        dw2, tmp = self._z(Cout, Kp), None
        ldx = dx.stride(0)
        for n0, n1 in self._chunks(N, HW, Kp):
            r0, r1 = n0 * HW, n1 * HW
            cols = ops.im2col3x3(x[r0:r1], (HW * ld, W * ld, ld, 1), self._e(r1 - r0, Kp), n1 - n0, H, W, Cin, 1)
            if n0 == 0:
                ops.gemm_tn(dz[r0:r1], cols, dw2)
            else:
                tmp = self._e(Cout, Kp, dtype=F32) if tmp is None else tmp
                ops.axpy(dw2, ops.gemm_tn(dz[r0:r1], cols, tmp))
            del cols
            dcols = ops.gemm_nt(dz[r0:r1], w2t, self._e(r1 - r0, Kp, dtype=F32))
            ops.col2im3x3(dcols, dx[r0:r1], (HW * ldx, W * ldx, ldx, 1), n1 - n0, H, W, Cin, 1)
        ops.conv3x3_unpack_grad(dw2, G[pre + ".conv.weight"])

    # ------------------------------------------------------------------ the trunk (UPerHead._forward_feature)
    def forward_feature(self, xs, shapes, P, training, reduce=None):
        """xs: the input maps (rows_i, Cin_i) ACT channels-last; shapes: (N, H_i, W_i) -> feat (rows_0, channels) ACT, context"""
        h = self.h
        self.P, self.training, self.reduce = P, training, reduce
        self.dev = xs[0].device
        Cc, L = h.channels, len(xs)
        N = shapes[0][0]
        # the BN layers' global row counts: one exchange (and one host sync) per forward, not one per layer
        local = sorted(set([n * hh * ww for n, hh, ww in shapes] + [N * s * s for s in h.pool_scales]))
        if training and reduce is not None:
            glob = reduce(torch.tensor(local, device=self.dev, dtype=torch.float64)).tolist()
        else:
            glob = [float(r) for r in local]
        self._counts = dict(zip(local, glob))
        ctx = dict(shapes=shapes, xs=xs)
        # PPM + bottleneck on the last map
        _, H3, W3 = shapes[-1]
        x3 = xs[-1]
        Cin3 = x3.shape[1]
        Ccat = Cin3 + len(h.pool_scales) * Cc
        cat = self._e(x3.shape[0], Ccat)
        ops.copy_rows(x3, cat, Cin3)
        ppm = []
        for j, s in enumerate(h.pool_scales):
            pooled = ops.adaptive_avg_pool_fwd(x3, self._e(N * s * s, Cin3), N, H3, W3, s)
            po, c = self._cm1_fwd(pooled, "psp_modules.%d.1" % j)
            ops.resize_bilinear_fwd(po, cat[:, Cin3 + j * Cc:Cin3 + (j + 1) * Cc], N, s, s, H3, W3)
            ppm.append(c)
        lat3, cb = self._cm3_fwd(cat, N, H3, W3, "bottleneck")
        ctx.update(ppm=ppm, bottleneck=cb)
        # laterals and the top-down path
        lats, lc = [], []
        for i in range(L - 1):
            o, c = self._cm1_fwd(xs[i], "lateral_convs.%d" % i)
            lats.append(o)
            lc.append(c)
        lats.append(lat3)
        for i in range(L - 1, 0, -1):
            ops.resize_bilinear_fwd(lats[i], lats[i - 1], N, shapes[i][1], shapes[i][2], shapes[i - 1][1], shapes[i - 1][2], accumulate=True)
        # fpn convs, resized into the concatenation, fpn_bottleneck
        _, H0, W0 = shapes[0]
        fcat = self._e(xs[0].shape[0], L * Cc)
        fc, fouts = [], []
        for i in range(L - 1):
            o, c = self._cm3_fwd(lats[i], N, shapes[i][1], shapes[i][2], "fpn_convs.%d" % i, out=fcat[:, :Cc] if i == 0 else None)
            fouts.append(o)
            fc.append(c)
        fouts.append(lats[-1])
        for i in range(1, L):
            ops.resize_bilinear_fwd(fouts[i], fcat[:, i * Cc:(i + 1) * Cc], N, shapes[i][1], shapes[i][2], H0, W0)
        feat, cf = self._cm3_fwd(fcat, N, H0, W0, "fpn_bottleneck")
        ctx.update(lateral=lc, fpn=fc, fpn_bottleneck=cf)
        return feat, ctx

    def backward_feature(self, dfeat, ctx, G):
        """dfeat (rows_0, channels) f32 -> d(input maps) (rows_i, Cin_i) f32; parameter gradients into G (name -> f32 tensor, overwritten)"""
        h = self.h
        shapes, xs = ctx["shapes"], ctx["xs"]
        Cc, L = h.channels, len(xs)
        N = shapes[0][0]
        _, H0, W0 = shapes[0]
        dfcat = self._e(xs[0].shape[0], L * Cc, dtype=F32)
        self._cm3_bwd(dfeat, ctx["fpn_bottleneck"], "fpn_bottleneck", G, dfcat)
        dl = [None] * L
        for i in range(1, L):
            dl[i] = ops.resize_bilinear_bwd(dfcat[:, i * Cc:(i + 1) * Cc], self._e(N * shapes[i][1] * shapes[i][2], Cc, dtype=F32),
                                            N, shapes[i][1], shapes[i][2], H0, W0)
        dfpn = [dfcat[:, :Cc]] + dl[1:L - 1]
        for i in range(L - 1):
            d = self._e(xs[i].shape[0], Cc, dtype=F32)
            self._cm3_bwd(dfpn[i], ctx["fpn"][i], "fpn_convs.%d" % i, G, d)
            dl[i] = d
        for i in range(1, L):        # the top-down adds, in reverse
            ops.resize_bilinear_bwd(dl[i - 1], dl[i], N, shapes[i][1], shapes[i][2], shapes[i - 1][1], shapes[i - 1][2], accumulate=True)
        dxs = [self._cm1_bwd(dl[i], ctx["lateral"][i], "lateral_convs.%d" % i, G) for i in range(L - 1)]
        _, H3, W3 = shapes[-1]
        Cin3 = xs[-1].shape[1]
        dcat = self._e(xs[-1].shape[0], Cin3 + len(h.pool_scales) * Cc, dtype=F32)
        self._cm3_bwd(dl[-1], ctx["bottleneck"], "bottleneck", G, dcat)
        for j, s in enumerate(h.pool_scales):
            dpo = ops.resize_bilinear_bwd(dcat[:, Cin3 + j * Cc:Cin3 + (j + 1) * Cc], self._e(N * s * s, Cc, dtype=F32), N, s, s, H3, W3)
            dpooled = self._cm1_bwd(dpo, ctx["ppm"][j], "psp_modules.%d.1" % j, G)
            ops.adaptive_avg_pool_bwd(dpooled, dcat[:, :Cin3], N, H3, W3, s, accumulate=True)
        dxs.append(ops.copy_rows(dcat, self._e(xs[-1].shape[0], Cin3, dtype=F32), Cin3))
        return dxs

    # ------------------------------------------------------------------ cls_seg (Dropout2d + 1x1 conv with bias)
    def cls_fwd(self, feat, N, HW, wname, bname, mask):
        """feat (rows, channels) ACT -> logits (rows, Kp) f32 (columns K .. Kp zero), context"""
        self.dev = feat.device
        w, b = self.P[wname], self.P[bname]
        K = w.shape[0]
        Kp = ops.pad8(K)
        wp, wpt = self._w1(wname, Kp)
        bp = self._z(Kp)
        bp[:K].copy_(b)
        fd = feat if mask is None else ops.channel_scale(feat, mask, HW, self._e(*feat.shape))
        logits = ops.gemm_nt(fd, wp, self._e(feat.shape[0], Kp, dtype=F32), bias=bp)
        return logits, dict(fd=fd, wpt=wpt, K=K, Kp=Kp, mask=mask, HW=HW)

    def cls_bwd(self, dlogits, c, G, wname, bname):
        """dlogits (rows, Kp) f32 -> dfeat (rows, channels) f32; d weight / d bias into G"""
        K, Kp = c["K"], c["Kp"]
        dla = dlogits if self.act == F32 else ops.cast(dlogits, self._e(*dlogits.shape))
        dwp, dbp = self._z(Kp, c["fd"].shape[1]), self._z(Kp)
        ops.gemm_tn(dla, c["fd"], dwp, colsum=dbp)
        G[wname].view(K, -1).copy_(dwp[:K])
        G[bname].copy_(dbp[:K])
        dfd = ops.gemm_nt(dla, c["wpt"], self._e(dla.shape[0], c["wpt"].shape[0], dtype=F32))
        if c["mask"] is not None:
            ops.channel_scale(dfd, c["mask"], c["HW"], dfd)
        return dfd

    # ------------------------------------------------------------------ layouts
    def to_rows(self, f, dtype=None):
        """NCHW (B, C, H, W) f32 / bf16 -> (B*H*W, C) ACT (or dtype)"""
        B, Cc, H, W = f.shape
        self.dev = f.device
        return ops.nchw_to_tokens(f.contiguous(), self._e(B * H * W, Cc, dtype=dtype), B, H, W, 0)

    def to_nchw(self, x, B, H, W, C=None):
        """(B*H*W, ld) -> NCHW f32 (the first C channels)"""
        ld = x.shape[1]
        out = ops.tokens_to_nchw(x.contiguous(), torch.empty(B, ld, H, W, device=x.device, dtype=F32), B, H, W, 0)
        return out if C is None or C == ld else out[:, :C].contiguous()
