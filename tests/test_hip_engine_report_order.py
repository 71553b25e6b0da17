"""The order in which the engines report finished gradient groups to on_block_done (mtp_amd.engine_base: _burst_out and the two tails) --
what decides when the gradient exchange may start on a slice.  The expected lists (tests/golden/engine_report_order.json) were recorded
from the engines as they were before they shared EngineBase, on the shapes below."""
import json
import os

import pytest
import torch

import mtp_amd
import recipe
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def report_order(net, img, split_last):
    """one forward + backward straight through the engine -> (group ids in the order they were reported, the engine)"""
    eng = net._engine()
    feats, ctx = eng.forward(img, training=True, need_grad=True)
    G = {n: torch.zeros_like(p, dtype=torch.float32) for n, p in net.named_parameters()}
    order = []
    # (sqn: the grouped launches list what they covered in norm_covered only when they are asked for the norm)
    eng.backward(ctx, [torch.full_like(f, 1.0 / f.numel()) for f in feats], G, on_block_done=order.append, split_last=split_last,
                 sqn=torch.zeros(1, device=img.device))
    torch.cuda.synchronize()
    return order, eng


def vit_case():
    """depth 4, 128 channels, 2 heads, full attention every 2nd block, bf16; 2 x 256 x 256 at patch 16 = 512 tokens, a multiple of 128: the weight
    gradients go through the grouped kernel (ops.WgradQueue.add)"""
    net = mtp_amd.ViT_Win_RVSA_V3_WSZ7(img_size=256, embed_dim=128, depth=4, num_heads=2, interval=2, qkv_bias=True, use_abs_pos_emb=True,
                                       out_indices=[0, 1, 2, 3], precision="bf16", feature_dtype=torch.float32)
    net.load_state_dict(recipe.make_params(recipe.state_shapes(128, 4, 2, 2, img_size=256)), strict=False)
    return net.cuda().train(), recipe.make_input(2, 256, 256, seed=5).cuda()


def intern_case():
    """the configuration of test_hip_internimage's side-stream test"""
    net = mtp_amd.internimage_xl(drop_path_rate=0.0).cuda().train()
    return net, torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(3)).cuda()


def key(name, side, split_last):
    return "%s side=%d split_last=%d" % (name, int(side), int(split_last))


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "engine_report_order.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def vit():
    return vit_case()


@pytest.fixture(scope="module")
def intern():
    return intern_case()


@pytest.mark.parametrize("split_last", [False, True])
@pytest.mark.parametrize("side", [False, True, 2])
def test_vit_report_order(monkeypatch, expected, vit, side, split_last):
    from mtp_amd.engine import BackboneEngine
    monkeypatch.setattr(BackboneEngine, "wgrad_side_stream", side)
    order, eng = report_order(*vit, split_last)
    assert len(eng.norm_covered) > 0          # the grouped path was taken: not the report-after-every-block path of immediate launches
    assert order == expected[key("vit", side, split_last)]


@pytest.mark.parametrize("side", [False, True, 2])
def test_internimage_report_order(monkeypatch, expected, intern, side):
    from mtp_amd.engine_intern import InternEngine
    monkeypatch.setattr(InternEngine, "wgrad_side_stream", side)
    order, eng = report_order(*intern, False)
    assert len(eng.norm_covered) > 0
    assert order == expected[key("internimage", side, False)]
