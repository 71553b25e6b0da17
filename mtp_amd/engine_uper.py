"""Explicit forward / backward schedule of the UperNet decode head's trunk (mmseg UPerHead._forward_feature) on the layers of
engine_decode: PPM + bottleneck on the last map, the laterals and their top-down path, the FPN convs resized into one concatenation, fpn_bottleneck.
Adaptive pooling and the bilinear resizes are the kernels of csrc/decode_head.hip.  The classifier runs on the trunk's own grid (DecodeEngine's
logits_fwd / logits_bwd)."""
from . import ops
from .engine_decode import F32, DecodeEngine


def _cm(pre):
    """mmcv ConvModule `pre` -> (its conv weight's name, its BN prefix)"""
    return pre + ".conv.weight", pre + ".bn."


class UperEngine(DecodeEngine):
    # ------------------------------------------------------------------ the trunk (UPerHead._forward_feature)
    def forward_feature(self, xs, shapes, P, training, reduce=None):
        """xs: the input maps (rows_i, Cin_i) ACT channels-last; shapes: (N, H_i, W_i) -> feat (rows_0, channels) ACT, context"""
        h = self.h
        Cc, L = h.channels, len(xs)
        N = shapes[0][0]
        self.bind(P, training, reduce, xs[0].device, [n * hh * ww for n, hh, ww in shapes] + [N * s * s for s in h.pool_scales])
        ctx = dict(shapes=shapes, xs=xs, grid=shapes[0])
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
            po, c = self._cm1_fwd(pooled, *_cm("psp_modules.%d.1" % j))
            ops.resize_bilinear_fwd(po, cat[:, Cin3 + j * Cc:Cin3 + (j + 1) * Cc], N, s, s, H3, W3)
            ppm.append(c)
        lat3, cb = self._cm3_fwd(cat, N, H3, W3, *_cm("bottleneck"))
        ctx.update(ppm=ppm, bottleneck=cb)
        # laterals and the top-down path
        lats, lc = [], []
        for i in range(L - 1):
            o, c = self._cm1_fwd(xs[i], *_cm("lateral_convs.%d" % i))
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
            o, c = self._cm3_fwd(lats[i], N, shapes[i][1], shapes[i][2], *_cm("fpn_convs.%d" % i), out=fcat[:, :Cc] if i == 0 else None)
            fouts.append(o)
            fc.append(c)
        fouts.append(lats[-1])
        for i in range(1, L):
            ops.resize_bilinear_fwd(fouts[i], fcat[:, i * Cc:(i + 1) * Cc], N, shapes[i][1], shapes[i][2], H0, W0)
        feat, cf = self._cm3_fwd(fcat, N, H0, W0, *_cm("fpn_bottleneck"))
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
        self._cm3_bwd(dfeat, ctx["fpn_bottleneck"], G, dfcat)
        dl = [None] * L
        for i in range(1, L):
            dl[i] = ops.resize_bilinear_bwd(dfcat[:, i * Cc:(i + 1) * Cc], self._e(N * shapes[i][1] * shapes[i][2], Cc, dtype=F32),
                                            N, shapes[i][1], shapes[i][2], H0, W0)
        dfpn = [dfcat[:, :Cc]] + dl[1:L - 1]
        for i in range(L - 1):
            d = self._e(xs[i].shape[0], Cc, dtype=F32)
            self._cm3_bwd(dfpn[i], ctx["fpn"][i], G, d)
            dl[i] = d
        for i in range(1, L):        # the top-down adds, in reverse
            ops.resize_bilinear_bwd(dl[i - 1], dl[i], N, shapes[i][1], shapes[i][2], shapes[i - 1][1], shapes[i - 1][2], accumulate=True)
        dxs = [self._cm1_bwd(dl[i], ctx["lateral"][i], G) for i in range(L - 1)]
        _, H3, W3 = shapes[-1]
        Cin3 = xs[-1].shape[1]
        dcat = self._e(xs[-1].shape[0], Cin3 + len(h.pool_scales) * Cc, dtype=F32)
        self._cm3_bwd(dl[-1], ctx["bottleneck"], G, dcat)
        for j, s in enumerate(h.pool_scales):
            dpo = ops.resize_bilinear_bwd(dcat[:, Cin3 + j * Cc:Cin3 + (j + 1) * Cc], self._e(N * s * s, Cc, dtype=F32), N, s, s, H3, W3)
            dpooled = self._cm1_bwd(dpo, ctx["ppm"][j], G)
            ops.adaptive_avg_pool_bwd(dpooled, dcat[:, :Cin3], N, H3, W3, s, accumulate=True)
        dxs.append(ops.copy_rows(dcat, self._e(xs[-1].shape[0], Cin3, dtype=F32), Cin3))
        return dxs
