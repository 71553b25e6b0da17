"""Explicit forward / backward schedule of the change-detection decoder (the reference's UNetHead, RS_Tasks_Finetune/Change_Detection/opencd/models/
decode_heads/unet_head.py) on libmtp_hip.so.

Built on UperEngine's pieces: the 3x3 ConvModules (im2col + NT GEMM in sample chunks, BatchNorm / SyncBN + ReLU), the classifier, the layout changes.
What is new is the decoder's data movement, the kernels of csrc/unet_head.hip: one launch writes a block's conv input (x nearest x2 | skip resized
bilinearly), one gather pair undoes it.  The classifier runs BEFORE the final x2 bilinear resize (Dropout2d scales per (sample, channel) and the
bilinear weights sum to one, so it commutes with the 1x1 conv and its bias): 4x fewer GEMM rows, and the resize moves 8 logit columns, not 64.
"""
import re

import torch

from . import ops
from .engine_uper import F32, UperEngine

_SEQ = re.compile(r"^(blocks\.\d+\.conv[12])\.([01])\.(.+)$")


def _alias(d):
    """the reference's nn.Sequential(conv, norm, relu) names -> also under the ConvModule names (`.conv.` / `.bn.`) UperEngine's layers look up; the
    tensors are shared, so statistics and gradients written through either name land in the same storage"""
    out = dict(d)
    for k, v in d.items():
        m = _SEQ.match(k)
        if m:
            out["%s.%s.%s" % (m.group(1), "conv" if m.group(2) == "0" else "bn", m.group(3))] = v
    return out


class UNetEngine(UperEngine):
    # ------------------------------------------------------------------ the decoder blocks (UNetHead.forward up to the last block)
    def forward_feature(self, xs, shapes, P, training, reduce=None):
        """xs: the (fused) input maps (rows_i, C_i) ACT channels-last in the backbone's order; shapes: (N, H_i, W_i) -> the last block's output
        (N * h * w, decoder_channels[-1]) ACT on its grid, context"""
        self.P, self.training, self.reduce = _alias(P), training, reduce
        self.dev = xs[0].device
        feats, shp = xs[::-1], shapes[::-1]
        N, h, w = shp[0]
        nb = self.h.n_blocks
        local = sorted(set(N * (h << (i + 1)) * (w << (i + 1)) for i in range(nb)))
        if training and reduce is not None:
            glob = reduce(torch.tensor(local, device=self.dev, dtype=torch.float64)).tolist()
        else:
            glob = [float(r) for r in local]
        self._counts = dict(zip(local, glob))
        x, blocks = feats[0], []
        for i in range(nb):
            skip = feats[i + 1] if i + 1 < len(feats) else None
            hs, ws = shp[i + 1][1:] if skip is not None else (0, 0)
            Cx, Cs = x.shape[1], 0 if skip is None else skip.shape[1]
            y = ops.unet_up_cat_fwd(x, skip, self._e(4 * N * h * w, Cx + Cs), N, h, w, hs, ws)
            a, c1 = self._cm3_fwd(y, N, 2 * h, 2 * w, "blocks.%d.conv1" % i)
            x, c2 = self._cm3_fwd(a, N, 2 * h, 2 * w, "blocks.%d.conv2" % i)
            blocks.append(dict(c1=c1, c2=c2, geom=(h, w, hs, ws), Cx=Cx, Cs=Cs))
            h, w = 2 * h, 2 * w
        return x, dict(blocks=blocks, N=N, grid=(h, w), n_in=len(xs))

    def backward_feature(self, dfeat, ctx, G):
        """dfeat (rows, decoder_channels[-1]) f32 -> d(input maps) (rows_i, C_i) f32 in the backbone's order; parameter gradients into G"""
        G = _alias(G)
        N, d = ctx["N"], dfeat
        dskips = []
        for i in range(len(ctx["blocks"]) - 1, -1, -1):
            b = ctx["blocks"][i]
            h, w, hs, ws = b["geom"]
            rows = 4 * N * h * w
            da = self._e(rows, b["c2"]["x"].shape[1], dtype=F32)
            self._cm3_bwd(d, b["c2"], "blocks.%d.conv2" % i, G, da)
            dy = self._e(rows, b["Cx"] + b["Cs"], dtype=F32)
            self._cm3_bwd(da, b["c1"], "blocks.%d.conv1" % i, G, dy)
            d, dsk = ops.unet_up_cat_bwd(dy, self._e(N * h * w, b["Cx"], dtype=F32), self._e(N * hs * ws, b["Cs"], dtype=F32) if b["Cs"] else None,
                                         N, h, w, hs, ws)
            if dsk is not None:
                dskips.append(dsk)
        # dskips: finest skip first; the head's own input (the coarsest map) last
        return dskips + [d]

    # ------------------------------------------------------------------ cls_seg, then the final x2 resize
    def logits_fwd(self, feat, N, h, w, mask):
        """-> logits (N * 2h * 2w, Kp) f32 on the 2x grid (what the reference's forward returns), context"""
        low, cc = self.cls_fwd(feat, N, h * w, "conv_seg.weight", "conv_seg.bias", mask)
        up = ops.resize_bilinear_fwd(low, self._e(4 * N * h * w, low.shape[1], dtype=F32), N, h, w, 2 * h, 2 * w)
        return up, dict(cc=cc, geom=(N, h, w))

    def logits_bwd(self, dup, c, G):
        """dup (N * 2h * 2w, Kp) f32 -> d(last block's output) (N * h * w, channels) f32; d conv_seg into G"""
        N, h, w = c["geom"]
        dlow = ops.resize_bilinear_bwd(dup, self._e(N * h * w, dup.shape[1], dtype=F32), N, h, w, 2 * h, 2 * w)
        return self.cls_bwd(dlow, c["cc"], G, "conv_seg.weight", "conv_seg.bias")
