"""The layers the decode heads' schedules (engine_uper, engine_unet; DESIGN sections 10 and 12) are made of, on libmtp_hip.so.

Every map is channels-last (rows = N*H*W, C).  Convolutions are GEMMs: 1x1 = mtp_gemm_nt on the rows, 3x3 = mtp_im2col3x3 + mtp_gemm_nt, worked in
sample chunks so the column buffer stays under COLS_BUDGET bytes; their gradients are mtp_gemm_tn (weights) and mtp_gemm_nt + mtp_col2im3x3 (data).
BatchNorm + ReLU, bilinear resize, Dropout2d and the segmentation loss are the kernels of csrc/decode_head.hip.  ACT (the GEMM operands, the BN
outputs) is f32 in 'fp32' mode and bf16 in 'bf16' mode; BN statistics, the logits and every gradient buffer are f32.

A layer is named by its parameters: the conv weight's name and the BN prefix (`bottleneck.conv.weight` / `bottleneck.bn.` under mmcv's ConvModule,
`blocks.0.conv1.0.weight` / `blocks.0.conv1.1.` under the reference UNet's nn.Sequential); the forward keeps both in the layer's context.

SyncBN: `reduce` (a callable that sums an f32 tensor over the ranks, in place, and returns it) is applied to each BN layer's (sum x, sum x^2, count)
between the statistics and the apply launch, and to (sum dy', sum dy' xhat) in the backward -- what torch.nn.SyncBatchNorm exchanges.

A schedule implements forward_feature(xs, shapes, P, training, reduce) -> (feat, ctx) with ctx["grid"] = feat's (N, h, w), and
backward_feature(dfeat, ctx, G); logits_fwd / logits_bwd are the classifier on that grid unless the schedule overrides them.
"""
import torch

from . import ops

F32 = torch.float32


class DecodeEngine:
    COLS_BUDGET = 256 << 20      # bytes of im2col columns (or of their gradient) per chunk

    def __init__(self, head, precision="fp32"):
        self.h = head
        self.act = F32 if precision == "fp32" else torch.bfloat16

    def bind(self, P, training, reduce, device, rows):
        """the run's state, set here and nowhere else.  P: name -> parameter / buffer; rows: the BN layers' local row counts, whose global counts
        take one exchange (and one host sync) per forward, not one per layer"""
        self.P, self.training, self.reduce, self.dev = P, training, reduce, device
        local = sorted(set(rows))
        if training and reduce is not None:
            glob = reduce(torch.tensor(local, device=device, dtype=torch.float64)).tolist()
        else:
            glob = [float(r) for r in local]
        self._counts = dict(zip(local, glob))

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
    def _bn_fwd(self, z, b, out):
        """z (rows, C) ACT conv output -> out (rows, C) ACT (a column slice is fine); returns what the backward needs"""
        P, C = self.P, z.shape[1]
        mean, rstd = self._e(C, dtype=F32), self._e(C, dtype=F32)
        if self.training:
            # two passes: a first mean, then the sums centred on it (exact variance when |mean| >> std); SyncBN all-reduces both
            count = self._counts[z.shape[0]]
            s1 = ops.bn_sums(z)
            if self.reduce is not None:
                s1 = self.reduce(s1)
            center = self._e(C, dtype=F32)
            ops.bn_finalize(s1, count, None, None, center, rstd)
            sums = ops.bn_sums(z, center)
            if self.reduce is not None:
                sums = self.reduce(sums)
            ops.bn_finalize(sums, count, P[b + "running_mean"], P[b + "running_var"], mean, rstd, momentum=0.1, eps=1e-5, center=center)
            P[b + "num_batches_tracked"].add_(1)
        else:
            count = 0.0
            ops.bn_finalize(None, 0.0, P[b + "running_mean"], P[b + "running_var"], mean, rstd, eps=1e-5)
        ops.bn_apply(z, mean, rstd, P[b + "weight"], P[b + "bias"], out, relu=True)
        return (z, mean, rstd, count, b)

    def _bn_bwd(self, dy, saved, G):
        """dy (rows, C) f32 -> dz (rows, C) ACT; d gamma / d beta (this rank's sums) into G"""
        z, mean, rstd, count, b = saved
        P, C = self.P, z.shape[1]
        sums = ops.bn_bwd_sums(dy, z, mean, rstd, P[b + "weight"], P[b + "bias"])
        G[b + "bias"].copy_(sums[:C])
        G[b + "weight"].copy_(sums[C:])
        if not self.training:
            sums = None
        elif self.reduce is not None:
            sums = self.reduce(sums.clone())
        return ops.bn_bwd_dx(dy, z, mean, rstd, P[b + "weight"], P[b + "bias"], sums, count, self._e(*z.shape))

    # ------------------------------------------------------------------ ConvModules (conv without bias -> BN -> ReLU)
    def _cm1_fwd(self, x, wname, b, out=None):
        """1x1: x (rows, Cin) ACT -> (rows, C) ACT"""
        wp, wpt = self._w1(wname)
        z = ops.gemm_nt(x, wp, self._e(x.shape[0], wp.shape[0]))
        out = self._e(*z.shape) if out is None else out
        return out, dict(x=x, wpt=wpt, w=wname, bn=self._bn_fwd(z, b, out))

    def _cm1_bwd(self, dy, c, G, need_dx=True):
        dz = self._bn_bwd(dy, c["bn"], G)
        ops.gemm_tn(dz, c["x"], G[c["w"]].view(dz.shape[1], -1))
        return ops.gemm_nt(dz, c["wpt"], self._e(dz.shape[0], c["wpt"].shape[0], dtype=F32)) if need_dx else None

    def _chunks(self, N, HW, Kp):
        per = max(1, self.COLS_BUDGET // max(1, HW * Kp * 4))
        return [(n0, min(N, n0 + per)) for n0 in range(0, N, per)]

    def _cm3_fwd(self, x, N, H, W, wname, b, out=None):
        """3x3 (padding 1): x (N*H*W, Cin) ACT (a column slice is fine) -> (rows, C) ACT"""
        w2, w2t = self._w3(wname)
        Cin, ld, HW = x.shape[1], x.stride(0), H * W
        z = self._e(x.shape[0], w2.shape[0])
        for n0, n1 in self._chunks(N, HW, w2.shape[1]):
            cols = ops.im2col3x3(x[n0 * HW:n1 * HW], (HW * ld, W * ld, ld, 1), self._e((n1 - n0) * HW, w2.shape[1]), n1 - n0, H, W, Cin, 1)
            ops.gemm_nt(cols, w2, z[n0 * HW:n1 * HW])
        out = self._e(*z.shape) if out is None else out
        return out, dict(x=x, w2t=w2t, geom=(N, H, W), w=wname, bn=self._bn_fwd(z, b, out))

    def _cm3_bwd(self, dy, c, G, dx):
        """dx: (rows, Cin) f32 (a column slice is fine) = the data gradient"""
        dz = self._bn_bwd(dy, c["bn"], G)
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
        ops.conv3x3_unpack_grad(dw2, G[c["w"]])

    # ------------------------------------------------------------------ cls_seg (Dropout2d + 1x1 conv with bias)
    def cls_fwd(self, feat, N, HW, wname, bname, mask):
        """feat (rows, channels) ACT -> logits (rows, Kp) f32 (columns K .. Kp zero), context"""
        w, b = self.P[wname], self.P[bname]
        K = w.shape[0]
        Kp = ops.pad8(K)
        wp, wpt = self._w1(wname, Kp)
        bp = self._z(Kp)
        bp[:K].copy_(b)
        fd = feat if mask is None else ops.channel_scale(feat, mask, HW, self._e(*feat.shape))
        logits = ops.gemm_nt(fd, wp, self._e(feat.shape[0], Kp, dtype=F32), bias=bp)
        return logits, dict(fd=fd, wpt=wpt, K=K, Kp=Kp, mask=mask, HW=HW, w=wname, b=bname)

    def cls_bwd(self, dlogits, c, G):
        """dlogits (rows, Kp) f32 -> dfeat (rows, channels) f32; d weight / d bias into G"""
        K, Kp = c["K"], c["Kp"]
        dla = dlogits if self.act == F32 else ops.cast(dlogits, self._e(*dlogits.shape))
        dwp, dbp = self._z(Kp, c["fd"].shape[1]), self._z(Kp)
        ops.gemm_tn(dla, c["fd"], dwp, colsum=dbp)
        G[c["w"]].view(K, -1).copy_(dwp[:K])
        G[c["b"]].copy_(dbp[:K])
        dfd = ops.gemm_nt(dla, c["wpt"], self._e(dla.shape[0], c["wpt"].shape[0], dtype=F32))
        if c["mask"] is not None:
            ops.channel_scale(dfd, c["mask"], c["HW"], dfd)
        return dfd

    def logits_fwd(self, feat, grid, mask, wname, bname):
        """feat on `grid` = (N, h, w) -> (logit rows (rows, Kp) f32, the grid they live on, context)"""
        logits, c = self.cls_fwd(feat, grid[0], grid[1] * grid[2], wname, bname, mask)
        return logits, grid, c

    def logits_bwd(self, dlogits, c, G):
        return self.cls_bwd(dlogits, c, G)

    # ------------------------------------------------------------------ layouts
    def to_rows(self, f, dtype=None):
        """NCHW (B, C, H, W) f32 / bf16 -> (B*H*W, C) ACT (or dtype)"""
        B, Cc, H, W = f.shape
        return ops.nchw_to_tokens(f.contiguous(), torch.empty(B * H * W, Cc, device=f.device, dtype=dtype or self.act), B, H, W, 0)

    @staticmethod
    def to_nchw(x, B, H, W, C=None):
        """(B*H*W, ld) -> NCHW f32 (the first C channels)"""
        ld = x.shape[1]
        out = ops.tokens_to_nchw(x.contiguous(), torch.empty(B, ld, H, W, device=x.device, dtype=F32), B, H, W, 0)
        return out if C is None or C == ld else out[:, :C].contiguous()

    @staticmethod
    def padded_rows(logits):
        """NCHW logits (N, K, h, w) -> (N*h*w, Kp) f32 rows, columns K .. Kp zero: what the loss, the resize and cls_bwd read"""
        N, K, h, w = logits.shape
        Kp = ops.pad8(K)
        lp = torch.zeros(N, Kp, h, w, device=logits.device, dtype=F32)
        lp[:, :K] = logits
        return ops.nchw_to_tokens(lp, torch.empty(N * h * w, Kp, device=lp.device, dtype=F32), N, h, w, 0)
