"""The layers of the FCN mask head (convs.{i}.conv 3x3 + ReLU, upsample 2x2 / stride-2 ConvTranspose2d + ReLU, then the per-dataset 1x1 conv_logits
passed in from outside) on the layers of engine_decode, forward and backward.

The RoI features arrive as the RoIAlign kernel writes them, (R, S S, C) = rows (R S S, C), channel last: the layout the convolutions work in.  A 3x3
conv is mtp_im2col3x3 + gemm_nt with the bias in the epilogue; ReLU is bn_apply with identity statistics (as in engine_roi); the deconvolution is
ONE gemm_nt against the ConvT pack of the FPN tail, whose (rows, 4 C) output read as (4 rows, C) holds the 2S x 2S map in quad order (pixel, tap).
ReLU and the 1x1 conv_logits are pointwise, so they run in quad order; only the logits are re-laid, to (R, Kp, 2S, 2S) with Kp = K padded to 8, by
tokens_to_nchw.  ACT is f32 in 'fp32' mode and bf16 in 'bf16' mode; the logits and every gradient are f32.

The weight images (w2 / w2T of every conv, wg / wgT of the deconvolution) are packed once per weight version and kept in the head's cache."""
import torch

from . import ops
from .engine_decode import F32, DecodeEngine


class MaskConvEngine(DecodeEngine):
    def __init__(self, head, precision="fp32", cache=None):
        super().__init__(head, precision)
        self.cache = {} if cache is None else cache

    def _images(self, P):
        """{conv weight name: (w2, w2T)}, 'upsample.weight': (wg, wgT)"""
        names = [n for n in P if n.endswith("weight")]
        key = (self.act,) + tuple((n, P[n].data_ptr(), P[n]._version) for n in names)
        if self.cache.get("key") != key:
            img = {}
            for n in names:
                w = P[n].detach().contiguous()
                if n.startswith("upsample."):
                    Cin, Cout = w.shape[:2]
                    img[n] = (self._e(4 * Cout, Cin), self._e(Cin, 4 * Cout))
                    ops.convt_pack(w, *img[n])
                else:
                    Kp = ops.pad8(9 * w.shape[1])
                    img[n] = (self._e(w.shape[0], Kp), self._e(Kp, w.shape[0]))
                    ops.conv3x3_pack(w, *img[n])
            self.cache.update(key=key, images=img, packs=self.cache.get("packs", 0) + 1)
        return self.cache["images"]

    def _relu(self, z):
        mean, one = self._z(z.shape[1]), torch.ones(z.shape[1], device=self.dev, dtype=F32)      # mean 0, rstd 1, gamma 1, beta 0: y = relu(z)
        return ops.bn_apply(z, mean, one, one, mean, self._e(*z.shape), relu=True), (mean, one)

    def _relu_bwd(self, dy, z, ident):
        mean, one = ident
        return ops.bn_bwd_dx(dy, z, mean, one, one, mean, None, 0.0, self._e(*z.shape))

    def _cols(self, x, n0, n1, S, Kp):
        Cin, ld, HW = x.shape[1], x.stride(0), S * S
        return ops.im2col3x3(x[n0 * HW:n1 * HW], (HW * ld, S * ld, ld, 1), self._e((n1 - n0) * HW, Kp), n1 - n0, S, S, Cin, 1)

    def head_rows(self, x, R, S, P):
        """x (R S S, Cin) f32 -> (feature rows ACT, context): after the convs (R S S, C); with the deconvolution (4 R S S, C) in quad order"""
        self.P, self.dev = P, x.device
        img = self._images(P)
        convs, cur = [], x
        n_convs = sum(1 for n in P if n.startswith("convs.") and n.endswith("weight"))
        for i in range(n_convs):
            name = "convs.%d.conv." % i
            w2, w2t = img[name + "weight"]
            z = self._e(cur.shape[0], w2.shape[0])
            for n0, n1 in self._chunks(R, S * S, w2.shape[1]):
                ops.gemm_nt(self._cols(cur, n0, n1, S, w2.shape[1]), w2, z[n0 * S * S:n1 * S * S], bias=P[name + "bias"].detach())
            y, ident = self._relu(z)
            convs.append(dict(x=cur, z=z, ident=ident, name=name, w2t=w2t))
            cur = y
        if cur is x and self.act != F32:
            cur = ops.cast(x, self._e(*x.shape))
        c = dict(convs=convs, R=R, S=S, up=None)
        if "upsample.weight" in P:
            wg, wgT = img["upsample.weight"]
            Cout = wg.shape[0] // 4
            z = ops.gemm_nt(cur, wg, self._e(cur.shape[0], 4 * Cout), bias=P["upsample.bias"].detach(), bias_mod=Cout).view(-1, Cout)
            y, ident = self._relu(z)
            c["up"] = dict(x=cur, z=z, ident=ident, wgT=wgT)
            cur = y
        return cur, c

    def logits_rows(self, feat, w, b):
        """the 1x1 conv_logits on feature rows -> (rows, Kp) f32, columns K .. Kp zero"""
        K, Cc = w.shape[0], w.shape[1]
        Kp = ops.pad8(K)
        wp, wpt = self._e(Kp, Cc), self._e(Cc, Kp)
        ops.pack_rows_padded(w.detach().reshape(K, Cc).contiguous(), wp, wpt)
        bp = self._z(Kp)
        if b is not None:
            bp[:K].copy_(b.detach())
        return ops.gemm_nt(feat, wp, self._e(feat.shape[0], Kp, dtype=F32), bias=bp), dict(feat=feat, wpt=wpt, K=K, Kp=Kp)

    def to_maps(self, rows, c):
        """rows (., ld) f32 in the head's output order -> (R, ld, M, M) f32, M = 2S after the deconvolution, else S"""
        R, S, ld = c["R"], c["S"], rows.shape[1]
        if c["up"] is None:
            return ops.tokens_to_nchw(rows, self._e(R, ld, S, S, dtype=F32), R, S, S, 0)
        return ops.tokens_to_nchw(rows, self._e(R, ld, 2 * S, 2 * S, dtype=F32), R, S, S, 1)

    def to_rows_like(self, maps, c):
        """the inverse of to_maps: (R, ld, M, M) f32 -> rows (., ld) f32"""
        R, S, ld = c["R"], c["S"], maps.shape[1]
        if c["up"] is None:
            return ops.nchw_to_tokens(maps, self._e(R * S * S, ld, dtype=F32), R, S, S, 0)
        return ops.nchw_to_tokens(maps, self._e(4 * R * S * S, ld, dtype=F32), R, S, S, 1)

    def logits_bwd_rows(self, dlogits, lc, G, names):
        """dlogits (rows, Kp) f32 -> d feature rows f32; names: the keys of G for conv_logits' weight and bias (None: no bias)"""
        K, Kp, feat = lc["K"], lc["Kp"], lc["feat"]
        da = dlogits if self.act == F32 else ops.cast(dlogits, self._e(*dlogits.shape))
        dwp, dbp = self._z(Kp, feat.shape[1]), self._z(Kp)
        ops.gemm_tn(da, feat, dwp, colsum=dbp)
        G[names[0]].view(K, -1).copy_(dwp[:K])
        if names[1] is not None:
            G[names[1]].copy_(dbp[:K])
        return ops.gemm_nt(da, lc["wpt"], self._e(da.shape[0], feat.shape[1], dtype=F32))

    def head_bwd(self, dfeat, c, G, need_dx=True):
        """dfeat: the gradient of head_rows' output, f32 -> dx (R S S, Cin) f32 (None without need_dx); the parameter gradients overwrite G"""
        R, S = c["R"], c["S"]
        dy = dfeat
        if c["up"] is not None:
            u = c["up"]
            dz = self._relu_bwd(dy, u["z"], u["ident"])
            Cout = dz.shape[1]
            dzr = dz.view(-1, 4 * Cout)
            dwg = self._z(4 * Cout, u["x"].shape[1])
            ops.gemm_tn(dzr, u["x"], dwg)
            ops.convt_unpack_grad(dwg, G["upsample.weight"])
            ops.colsum(dz, G["upsample.bias"])
            dy = ops.gemm_nt(dzr, u["wgT"], self._e(dzr.shape[0], u["x"].shape[1], dtype=F32))
        for i in reversed(range(len(c["convs"]))):
            L = c["convs"][i]
            dz = self._relu_bwd(dy, L["z"], L["ident"])
            x, w2t = L["x"], L["w2t"]
            Kp, Cout, HW = w2t.shape[0], w2t.shape[1], S * S
            dw2, db, tmp = self._z(Cout, Kp), self._z(Cout), None
            last = i == 0
            dx = self._e(x.shape[0], x.shape[1], dtype=F32) if (need_dx or not last) else None
            for n0, n1 in self._chunks(R, HW, Kp):
                r0, r1 = n0 * HW, n1 * HW
                cols = self._cols(x, n0, n1, S, Kp)
                if n0 == 0:
                    ops.gemm_tn(dz[r0:r1], cols, dw2, colsum=db)
                else:
                    tmp = self._e(Cout, Kp, dtype=F32) if tmp is None else tmp
                    ops.axpy(dw2, ops.gemm_tn(dz[r0:r1], cols, tmp, colsum=db))
                del cols
                if dx is not None:
                    dcols = ops.gemm_nt(dz[r0:r1], w2t, self._e(r1 - r0, Kp, dtype=F32))
                    ldx = dx.stride(0)
                    ops.col2im3x3(dcols, dx[r0:r1], (HW * ldx, S * ldx, ldx, 1), n1 - n0, S, S, x.shape[1], 1)
            ops.conv3x3_unpack_grad(dw2, G[L["name"] + "weight"])
            G[L["name"] + "bias"].copy_(db)
            dy = dx
        return dy
