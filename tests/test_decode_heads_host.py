"""The decode heads' structure (no GPU): one base head, one layer engine with two schedules, and no module that reaches into a sibling's."""
import ast
import glob
import os

import pytest

import mtp_amd
from mtp_amd import UNetHead, UPerHead
from mtp_amd.decode_heads.base import BaseDecodeHead
from mtp_amd.engine_decode import DecodeEngine
from mtp_amd.engine_unet import UNetEngine
from mtp_amd.engine_uper import UperEngine

PKG = os.path.dirname(mtp_amd.__file__)


def _imported_modules(path):
    """the module names a source file imports from (`from X import ...`, dots of relative imports dropped) or imports (`import X`)"""
    with open(path) as f:
        tree = ast.parse(f.read())
    names = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            names += [node.module or ""] + ["%s.%s" % (node.module or "", a.name) for a in node.names]
        elif isinstance(node, ast.Import):
            names += [a.name for a in node.names]
    return names


def test_heads_share_one_base_and_the_engines_one_layer_class():
    assert issubclass(UPerHead, BaseDecodeHead) and issubclass(UNetHead, BaseDecodeHead)
    assert issubclass(UperEngine, DecodeEngine) and issubclass(UNetEngine, DecodeEngine) and not issubclass(UNetEngine, UperEngine)
    assert UPerHead.engine is UperEngine and UNetHead.engine is UNetEngine
    for name in ("forward_feature", "backward_feature"):        # each schedule is its own
        assert name in vars(UperEngine) and name in vars(UNetEngine) and name not in vars(DecodeEngine)
    assert DecodeEngine.COLS_BUDGET == 256 << 20


def test_unet_head_refusal_names_the_unet_head():
    with pytest.raises(NotImplementedError, match="UNetHead"):
        UNetHead(encoder_channels=[8] * 4, decoder_channels=[32, 16, 8, 8], n_blocks=4, num_classes=2, align_corners=True)
    with pytest.raises(NotImplementedError, match="UPerHead"):
        UPerHead(in_channels=[8] * 4, channels=8, num_classes=2, align_corners=True)


def test_unet_head_and_segmentors_import_no_sibling_head_or_engine():
    files = [os.path.join(PKG, "decode_heads", "unet_head.py")] + sorted(glob.glob(os.path.join(PKG, "segmentors", "*.py")))
    assert len(files) >= 3
    for path in files:
        mods = _imported_modules(path)
        assert not any("uper_head" in m or "engine_uper" in m for m in mods), (path, mods)
        if os.path.basename(os.path.dirname(path)) == "segmentors":      # (the head itself names its own schedule, engine_unet)
            assert not any("engine" in m for m in mods), (path, mods)
