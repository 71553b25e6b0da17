"""Explicit forward / backward schedule of the change-detection decoder (the reference's UNetHead, RS_Tasks_Finetune/Change_Detection/opencd/models/
decode_heads/unet_head.py) on the layers of engine_decode.

The decoder's own data movement are the kernels of csrc/unet_head.hip: one launch writes a block's conv input (x nearest x2 | skip resized
bilinearly), one gather pair undoes it.  The classifier runs BEFORE the final x2 bilinear resize (Dropout2d scales per (sample, channel) and the
bilinear weights sum to one, so it commutes with the 1x1 conv and its bias): 4x fewer GEMM rows, and the resize moves 8 logit columns, not 64.
"""
from . import ops
from .engine_decode import F32, DecodeEngine


def _seq(i, j):
    """the reference's nn.Sequential(conv, norm, relu) `blocks.i.convj` -> (its conv weight's name, its BN prefix)"""
    return "blocks.%d.conv%d.0.weight" % (i, j), "blocks.%d.conv%d.1." % (i, j)


class UNetEngine(DecodeEngine):
    # ------------------------------------------------------------------ the decoder blocks (UNetHead.forward up to the last block)
    def forward_feature(self, xs, shapes, P, training, reduce=None):
        """xs: the (fused) input maps (rows_i, C_i) ACT channels-last in the backbone's order; shapes: (N, H_i, W_i) -> the last block's output
        (N * h * w, decoder_channels[-1]) ACT on its grid, context"""
        feats, shp = xs[::-1], shapes[::-1]
        N, h, w = shp[0]
        nb = self.h.n_blocks
        self.bind(P, training, reduce, xs[0].device, [N * (h << (i + 1)) * (w << (i + 1)) for i in range(nb)])
        x, blocks = feats[0], []
        for i in range(nb):
            skip = feats[i + 1] if i + 1 < len(feats) else None
            hs, ws = shp[i + 1][1:] if skip is not None else (0, 0)
            Cx, Cs = x.shape[1], 0 if skip is None else skip.shape[1]
            y = ops.unet_up_cat_fwd(x, skip, self._e(4 * N * h * w, Cx + Cs), N, h, w, hs, ws)
            a, c1 = self._cm3_fwd(y, N, 2 * h, 2 * w, *_seq(i, 1))
            x, c2 = self._cm3_fwd(a, N, 2 * h, 2 * w, *_seq(i, 2))
            blocks.append(dict(c1=c1, c2=c2, geom=(h, w, hs, ws), Cx=Cx, Cs=Cs))
            h, w = 2 * h, 2 * w
        return x, dict(blocks=blocks, grid=(N, h, w))

    def backward_feature(self, dfeat, ctx, G):
        """dfeat (rows, decoder_channels[-1]) f32 -> d(input maps) (rows_i, C_i) f32 in the backbone's order; parameter gradients into G"""
        N, d = ctx["grid"][0], dfeat
        dskips = []
        for b in ctx["blocks"][::-1]:
            h, w, hs, ws = b["geom"]
            rows = 4 * N * h * w
            da = self._e(rows, b["c2"]["x"].shape[1], dtype=F32)
            self._cm3_bwd(d, b["c2"], G, da)
            dy = self._e(rows, b["Cx"] + b["Cs"], dtype=F32)
            self._cm3_bwd(da, b["c1"], G, dy)
            d, dsk = ops.unet_up_cat_bwd(dy, self._e(N * h * w, b["Cx"], dtype=F32), self._e(N * hs * ws, b["Cs"], dtype=F32) if b["Cs"] else None,
                                         N, h, w, hs, ws)
            if dsk is not None:
                dskips.append(dsk)
        # dskips: finest skip first; the head's own input (the coarsest map) last
        return dskips + [d]

    # ------------------------------------------------------------------ cls_seg, then the final x2 resize
    def logits_fwd(self, feat, grid, mask, wname, bname):
        """-> logits (N * 2h * 2w, Kp) f32 on the 2x grid (what the reference's forward returns), that grid, context"""
        N, h, w = grid
        low, cc = self.cls_fwd(feat, N, h * w, wname, bname, mask)
        up = ops.resize_bilinear_fwd(low, self._e(4 * N * h * w, low.shape[1], dtype=F32), N, h, w, 2 * h, 2 * w)
        return up, (N, 2 * h, 2 * w), dict(cc=cc, geom=grid)

    def logits_bwd(self, dup, c, G):
        """dup (N * 2h * 2w, Kp) f32 -> d(last block's output) (N * h * w, channels) f32; d conv_seg into G"""
        N, h, w = c["geom"]
        dlow = ops.resize_bilinear_bwd(dup, self._e(N * h * w, dup.shape[1], dtype=F32), N, h, w, 2 * h, 2 * w)
        return self.cls_bwd(dlow, c["cc"], G)
