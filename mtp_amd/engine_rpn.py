"""The three convolutions of the RPN heads (rpn_conv 3x3 + ReLU, rpn_cls and rpn_reg 1x1) on the layers of engine_decode, forward and backward.

The weights are shared by the levels, so the levels' rows are stacked: one row per (level, image, y, x), level after level.  The 3x3 convolution is
im2col3x3 + gemm_nt per level (bias from the GEMM epilogue); ReLU is bn_apply with identity statistics over all rows at once; the two 1x1
convolutions are ONE gemm_nt over all rows with their (1 + D) A output channels padded to a multiple of 8 columns: columns 0 .. A are the logits,
A .. (1 + D) A the deltas (anchor-major, D each: six for the oriented head, four for the horizontal one; the widths are read off the weights).  ACT is f32 in 'fp32' mode and bf16 in 'bf16' mode; the logits, the deltas and every gradient are f32."""
import torch

from . import ops
from .engine_decode import F32, DecodeEngine

CONV, CLS, REG = "rpn_conv", "rpn_cls", "rpn_reg"


class RPNEngine(DecodeEngine):
    def forward_maps(self, feats, P):
        """feats: NCHW maps, one per level -> (out (rows, ldo) f32, context); level l owns rows ctx['row0'][l] .. of out"""
        self.P, self.dev = P, feats[0].device
        geoms = [(int(f.shape[0]), int(f.shape[2]), int(f.shape[3])) for f in feats]
        row0, rows = [], 0
        for N, H, W in geoms:
            row0.append(rows)
            rows += N * H * W
        xs = [self.to_rows(f) for f in feats]
        w2, w2t = self._w3(CONV + ".weight")
        feat = w2.shape[0]
        z = self._e(rows, feat)
        for x, (N, H, W), r in zip(xs, geoms, row0):
            HW = H * W
            for n0, n1 in self._chunks(N, HW, w2.shape[1]):
                cols = ops.im2col3x3(x[n0 * HW:n1 * HW], (HW * x.shape[1], W * x.shape[1], x.shape[1], 1), self._e((n1 - n0) * HW, w2.shape[1]), n1 - n0, H, W,
                                     x.shape[1], 1)
                ops.gemm_nt(cols, w2, z[r + n0 * HW:r + n1 * HW], bias=P[CONV + ".bias"])
        ident = (self._z(feat), torch.ones(feat, device=self.dev, dtype=F32))      # mean 0, rstd 1, gamma 1, beta 0: y = relu(z)
        y = ops.bn_apply(z, ident[0], ident[1], ident[1], ident[0], self._e(rows, feat), relu=True)
        wc = torch.cat([P[CLS + ".weight"].reshape(-1, feat), P[REG + ".weight"].reshape(-1, feat)], 0).contiguous()
        K = wc.shape[0]
        Kp = ops.pad8(K)
        wp, wpt = self._e(Kp, feat), self._e(feat, Kp)
        ops.pack_rows_padded(wc, wp, wpt)
        bp = self._z(Kp)
        bp[:K].copy_(torch.cat([P[CLS + ".bias"], P[REG + ".bias"]]))
        out = ops.gemm_nt(y, wp, self._e(rows, Kp, dtype=F32), bias=bp)
        return out, dict(xs=xs, geoms=geoms, row0=row0, z=z, y=y, ident=ident, w2t=w2t, wpt=wpt, K=K, Kp=Kp)

    def backward_maps(self, dout, c, G):
        """dout (rows, ldo) f32 -> the gradients of the input maps as f32 rows, one per level; the parameter gradients overwrite G"""
        P, K, Kp, y, z = self.P, c["K"], c["Kp"], c["y"], c["z"]
        A = P[CLS + ".weight"].shape[0]
        feat = y.shape[1]
        da = dout if self.act == F32 else ops.cast(dout, self._e(*dout.shape))
        dwp, dbp = self._z(Kp, feat), self._z(Kp)
        ops.gemm_tn(da, y, dwp, colsum=dbp)
        G[CLS + ".weight"].view(A, feat).copy_(dwp[:A])
        G[REG + ".weight"].view(K - A, feat).copy_(dwp[A:K])
        G[CLS + ".bias"].copy_(dbp[:A])
        G[REG + ".bias"].copy_(dbp[A:K])
        dy = ops.gemm_nt(da, c["wpt"], self._e(y.shape[0], feat, dtype=F32))
        mean, one = c["ident"]
        dz = ops.bn_bwd_dx(dy, z, mean, one, one, mean, None, 0.0, self._e(*z.shape))
        w2t = c["w2t"]
        Kp3 = w2t.shape[0]
        dw2, db, tmp, first = self._z(feat, Kp3), self._z(feat), None, True
        dxs = []
        for x, (N, H, W), r in zip(c["xs"], c["geoms"], c["row0"]):
            HW, Cin = H * W, x.shape[1]
            dx = self._e(N * HW, Cin, dtype=F32)
            for n0, n1 in self._chunks(N, HW, Kp3):
                r0, r1 = n0 * HW, n1 * HW
                cols = ops.im2col3x3(x[r0:r1], (HW * Cin, W * Cin, Cin, 1), self._e(r1 - r0, Kp3), n1 - n0, H, W, Cin, 1)
                if first:
                    ops.gemm_tn(dz[r + r0:r + r1], cols, dw2, colsum=db)
                    first = False
                else:
                    tmp = self._e(feat, Kp3, dtype=F32) if tmp is None else tmp
                    ops.axpy(dw2, ops.gemm_tn(dz[r + r0:r + r1], cols, tmp, colsum=db))
                del cols
                dcols = ops.gemm_nt(dz[r + r0:r + r1], w2t, self._e(r1 - r0, Kp3, dtype=F32))
                ops.col2im3x3(dcols, dx[r0:r1], (HW * Cin, W * Cin, Cin, 1), n1 - n0, H, W, Cin, 1)
            dxs.append(dx)
        ops.conv3x3_unpack_grad(dw2, G[CONV + ".weight"])
        G[CONV + ".bias"].copy_(db)
        return dxs
