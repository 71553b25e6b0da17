"""The fully connected layers of the RoI bbox head (shared_fcs.0 / .1 with ReLU, then fc_cls and fc_reg) on the layers of engine_decode, forward and
backward.  A Linear is gemm_nt with the bias in the epilogue; ReLU is bn_apply with identity statistics (as in engine_rpn); fc_cls and fc_reg are
ONE gemm_nt with their K + 1 + 5 output columns padded to a multiple of 8: columns 0 .. K are the logits, K + 1 .. K + 5 the deltas.

The RoI features arrive as (R, bins * C) rows in the kernel's order (bin, c); shared_fcs.0.weight is stored in the reference's flatten order
(c, ph, pw).  The weight IMAGE of the first layer is permuted once per weight version, not the activations; its gradient is permuted back.
ACT is f32 in 'fp32' mode and bf16 in 'bf16' mode; the logits, the deltas and every gradient are f32."""
import torch

from . import ops
from .engine_decode import F32, DecodeEngine

FC0, FC1 = "shared_fcs.0", "shared_fcs.1"


class RoIFCEngine(DecodeEngine):
    def __init__(self, head, precision="fp32", cache=None):
        super().__init__(head, precision)
        self.cache = {} if cache is None else cache      # the head's: the permuted image of shared_fcs.0.weight outlives one run

    def _first_image(self, w, bins):
        """(F, C * bins) in (c, bin) order -> (w (F, bins * C), wT (bins * C, F)) ACT in (bin, c) order"""
        key = (w.data_ptr(), w._version, self.act, bins)
        if self.cache.get("key") != key:
            F_, K0 = w.shape
            perm = w.detach().view(F_, K0 // bins, bins).permute(0, 2, 1).reshape(F_, K0).contiguous()
            wp, wpt = self._e(F_, K0), self._e(K0, F_)
            ops.pack_rows_padded(perm, wp, wpt)
            self.cache.update(key=key, images=(wp, wpt))
        return self.cache["images"]

    def _image(self, w):
        wp, wpt = self._e(*w.shape), self._e(w.shape[1], w.shape[0])
        ops.pack_rows_padded(w.detach().contiguous(), wp, wpt)
        return wp, wpt

    def _relu(self, z):
        ident = (self._z(z.shape[1]), torch.ones(z.shape[1], device=self.dev, dtype=F32))      # mean 0, rstd 1, gamma 1, beta 0: y = relu(z)
        return ops.bn_apply(z, ident[0], ident[1], ident[1], ident[0], self._e(*z.shape), relu=True), ident

    def forward_rows(self, x, bins, P, w_cls, b_cls, w_reg, b_reg):
        """x (R, bins * C) f32 in (bin, c) order -> (out (R, Kp) f32, context)"""
        self.P, self.dev = P, x.device
        xa = x if self.act == F32 else ops.cast(x, self._e(*x.shape))
        w0, w0t = self._first_image(P[FC0 + ".weight"], bins)
        z1 = ops.gemm_nt(xa, w0, self._e(x.shape[0], w0.shape[0]), bias=P[FC0 + ".bias"].detach())
        y1, ident = self._relu(z1)
        w1, w1t = self._image(P[FC1 + ".weight"])
        z2 = ops.gemm_nt(y1, w1, self._e(x.shape[0], w1.shape[0]), bias=P[FC1 + ".bias"].detach())
        y2, _ = self._relu(z2)
        wc = torch.cat([w_cls.detach(), w_reg.detach()], 0).contiguous()
        K = wc.shape[0]
        Kp = ops.pad8(K)
        wp, wpt = self._e(Kp, wc.shape[1]), self._e(wc.shape[1], Kp)
        ops.pack_rows_padded(wc, wp, wpt)
        bp = self._z(Kp)
        bp[:K].copy_(torch.cat([b_cls.detach(), b_reg.detach()]))
        out = ops.gemm_nt(y2, wp, self._e(x.shape[0], Kp, dtype=F32), bias=bp)
        return out, dict(x=xa, z1=z1, y1=y1, z2=z2, y2=y2, ident=ident, w0t=w0t, w1t=w1t, wpt=wpt, K=K, Kp=Kp, n_cls=w_cls.shape[0], bins=bins)

    def shared_rows(self, x, bins, P):
        """the two shared layers alone -> (R, fc_out) ACT"""
        self.P, self.dev = P, x.device
        xa = x if self.act == F32 else ops.cast(x, self._e(*x.shape))
        w0, _ = self._first_image(P[FC0 + ".weight"], bins)
        y1, _ = self._relu(ops.gemm_nt(xa, w0, self._e(x.shape[0], w0.shape[0]), bias=P[FC0 + ".bias"].detach()))
        w1, _ = self._image(P[FC1 + ".weight"])
        return self._relu(ops.gemm_nt(y1, w1, self._e(x.shape[0], w1.shape[0]), bias=P[FC1 + ".bias"].detach()))[0]

    def backward_rows(self, dout, c, G, names):
        """dout (R, Kp) f32 -> dx (R, bins * C) f32 in (bin, c) order; the parameter gradients overwrite G.  names: the keys of G for
        (fc_cls.weight, fc_cls.bias, fc_reg.weight, fc_reg.bias)"""
        K, Kp, n_cls = c["K"], c["Kp"], c["n_cls"]
        mean, one = c["ident"]
        F_ = c["y2"].shape[1]
        da = dout if self.act == F32 else ops.cast(dout, self._e(*dout.shape))
        dwp, dbp = self._z(Kp, F_), self._z(Kp)
        ops.gemm_tn(da, c["y2"], dwp, colsum=dbp)
        G[names[0]].copy_(dwp[:n_cls])
        G[names[1]].copy_(dbp[:n_cls])
        G[names[2]].copy_(dwp[n_cls:K])
        G[names[3]].copy_(dbp[n_cls:K])
        dy2 = ops.gemm_nt(da, c["wpt"], self._e(da.shape[0], F_, dtype=F32))
        dz2 = ops.bn_bwd_dx(dy2, c["z2"], mean, one, one, mean, None, 0.0, self._e(*c["z2"].shape))
        dw1, db1 = self._z(F_, c["y1"].shape[1]), self._z(F_)
        ops.gemm_tn(dz2, c["y1"], dw1, colsum=db1)
        G[FC1 + ".weight"].copy_(dw1)
        G[FC1 + ".bias"].copy_(db1)
        dy1 = ops.gemm_nt(dz2, c["w1t"], self._e(da.shape[0], c["y1"].shape[1], dtype=F32))
        dz1 = ops.bn_bwd_dx(dy1, c["z1"], mean, one, one, mean, None, 0.0, self._e(*c["z1"].shape))      # (both shared layers are fc_out wide)
        K0, bins = c["x"].shape[1], c["bins"]
        dw0, db0 = self._z(dz1.shape[1], K0), self._z(dz1.shape[1])
        ops.gemm_tn(dz1, c["x"], dw0, colsum=db0)
        G[FC0 + ".weight"].copy_(dw0.view(-1, bins, K0 // bins).permute(0, 2, 1).reshape(-1, K0))
        G[FC0 + ".bias"].copy_(db0)
        return ops.gemm_nt(dz1, c["w0t"], self._e(da.shape[0], K0, dtype=F32))
