"""mmdet's AnchorGenerator for the dense heads (rotated_detection/oriented_rcnn.py:24-29; anchor_head.py:167-202): the base anchors on the host in the
same float32 torch expressions, the grid and the inside flags by one launch per level (mtp_amd.ops.rpn_anchors), cached per shape key."""
import torch

from .. import ops
from ..registry import TASK_UTILS


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


@TASK_UTILS.register_module(name=["AnchorGenerator", "mmdet.AnchorGenerator"])
class AnchorGenerator:
    """AnchorGenerator(strides, ratios, scales, base_sizes=None, scale_major=True, use_box_type=False): center_offset 0.  Priors are plain (n, 4)
    float32 tensors x1, y1, x2, y2 whatever use_box_type says (there is no box class here)."""

    def __init__(self, strides, ratios, scales=None, base_sizes=None, scale_major=True, octave_base_scale=None, scales_per_octave=None, centers=None,
                 center_offset=0.0, use_box_type=False):
        if octave_base_scale is not None or scales_per_octave is not None:
            raise NotImplementedError("AnchorGenerator: octave_base_scale / scales_per_octave are not built (the MTP configs give scales)")
        if centers is not None or center_offset != 0:
            raise NotImplementedError("AnchorGenerator: centers and a non-zero center_offset are not built")
        if not scale_major:
            raise NotImplementedError("AnchorGenerator: scale_major=False is not built")
        if scales is None:
            raise ValueError("AnchorGenerator: scales is required")
        self.strides = [_pair(s) for s in strides]
        self.base_sizes = [min(s) for s in self.strides] if base_sizes is None else [int(b) for b in base_sizes]
        if len(self.base_sizes) != len(self.strides):
            raise ValueError("AnchorGenerator: as many base_sizes as strides")
        if len(self.strides) > ops.RPN_MAX_LEVELS:
            raise ValueError("AnchorGenerator: at most %d levels" % ops.RPN_MAX_LEVELS)
        self.scales, self.ratios = torch.tensor(scales, dtype=torch.float32), torch.tensor(ratios, dtype=torch.float32)
        self.use_box_type = use_box_type
        self.base_anchors = [self.gen_single_level_base_anchors(b) for b in self.base_sizes]
        self._cache = {}

    @property
    def num_base_priors(self):
        return [b.shape[0] for b in self.base_anchors]

    @property
    def num_base_anchors(self):
        return self.num_base_priors

    @property
    def num_levels(self):
        return len(self.strides)

    def gen_single_level_base_anchors(self, base_size):
        """(A, 4) float32 on the host, mmdet's expressions: ratios vary slowest"""
        w = h = base_size
        h_ratios = torch.sqrt(self.ratios)
        w_ratios = 1 / h_ratios
        ws = (w * w_ratios[:, None] * self.scales[None, :]).view(-1)
        hs = (h * h_ratios[:, None] * self.scales[None, :]).view(-1)
        return torch.stack([-0.5 * ws, -0.5 * hs, 0.5 * ws, 0.5 * hs], dim=-1)

    def priors_and_flags(self, featmap_sizes, pad_shape, img_shape, allowed_border, device):
        """per level (priors (H W A, 4) f32, inside flags (H W A) uint8) for one (feature-map sizes, shapes) key; computed once and kept.  The
        flags are anchor_head.py:192-201 (valid_flags) followed by mmdet's anchor_inside_flags."""
        if len(featmap_sizes) != self.num_levels:
            raise ValueError("AnchorGenerator: %d feature maps for %d levels" % (len(featmap_sizes), self.num_levels))
        device = torch.device(device)
        key = (tuple((int(h), int(w)) for h, w in featmap_sizes), tuple(int(v) for v in pad_shape[:2]), tuple(int(v) for v in img_shape[:2]),
               float(allowed_border), device.type, device.index)
        if key not in self._cache:
            out = []
            for (H, W), stride, base in zip(key[0], self.strides, self.base_anchors):
                n = H * W * base.shape[0]
                priors, flags = torch.empty(n, 4, device=device), torch.empty(n, device=device, dtype=torch.uint8)
                ops.rpn_anchors(base.to(device), H, W, stride, key[1], key[2], key[3], priors, flags)
                out.append((priors, flags))
            self._cache[key] = out
        return self._cache[key]

    def grid_priors(self, featmap_sizes, dtype=torch.float32, device="cuda", with_stride=False):
        if with_stride or dtype != torch.float32:
            raise NotImplementedError("AnchorGenerator.grid_priors: float32 priors without strides only")
        big = (1 << 30, 1 << 30)
        return [p for p, _ in self.priors_and_flags(featmap_sizes, big, big, -1, device)]

    def valid_flags(self, featmap_sizes, pad_shape, device="cuda"):
        return [f.bool() for _, f in self.priors_and_flags(featmap_sizes, pad_shape, pad_shape, -1, device)]
