"""CPU: scene classification's host side -- the ABI entries, the eleven reference configs through MODELS.build, the refusals, the head's
initialisation, Accuracy's host logic, and fixture f20(a) (tests/golden/make_cls_head.py: the reference's mmpretrain backbone file, then the restated
neck / head / loss in float64) against the project's CPU restatement of the backbone plus torch for the head."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mtp_amd
from conftest import GOLDEN, ROOT, rel_err
from mtp_amd import MODELS, Accuracy, GlobalAveragePooling, ImageClassifier, LinearClsHead
from oracle import vit_rvsa_oracle as O

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import recipe  # noqa: E402

TOL = 2e-5          # tests/test_oracle_golden.py's bound for f10: forward TOL, gradients 5 * TOL
CONFIGS = json.load(open(os.path.join(GOLDEN, "f20_cls_configs.json")))
ENTRIES = ("mtp_gap_fwd", "mtp_gap_bwd", "mtp_cls_ce", "mtp_cls_head_bwd", "mtp_cls_hits")


def test_abi_entries_are_bound_and_refuse_null_arguments():
    import ctypes as C
    from mtp_amd import _lib, ops
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        args = [0.0 if a is C.c_float else (None if (a is C.c_void_p or hasattr(a, "contents")) else 0) for a in _lib.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == -1, name
    for fn in ("gap_fwd", "gap_bwd", "cls_ce", "cls_head_bwd", "cls_hits"):
        assert callable(getattr(ops, fn))
    with pytest.raises(RuntimeError):          # no CPU fallback
        ops.gap_fwd(torch.zeros(1, 2, 3, 3))


def test_every_reference_config_builds():
    assert len(CONFIGS) == 11
    for name, cfg in CONFIGS.items():
        m = cfg["model"]
        assert m["type"] == "ImageClassifier" and m["backbone"]["type"] in ("RVSA_MTP", "InternImage"), name
        neck, head, ev = MODELS.build(m["neck"]), MODELS.build(m["head"]), MODELS.build(cfg["val_evaluator"])
        assert isinstance(neck, GlobalAveragePooling) and not list(neck.parameters())
        assert isinstance(head, LinearClsHead) and head.fc.weight.shape == (m["head"]["num_classes"], m["head"]["in_channels"])
        assert head.topk == (1, 5) and head.loss_weight == 1.0 and list(head.state_dict()) == ["fc.weight", "fc.bias"]
        assert isinstance(ev, Accuracy) and ev.topk == (1, 5) and ev.thrs == 0.0 and ev.counters is None


def test_vit_b_eurosat_model_dict_builds_as_a_whole_classifier():
    m = json.loads(json.dumps(CONFIGS["eurosat/vit-rvsa-b-224-mae-mtp_eurosat.py"]["model"]))
    assert m["backbone"]["type"] == "RVSA_MTP" and m["backbone"]["pretrained"]
    m["backbone"].update(type="RVSA_MTP_taps", pretrained=None)       # mmpretrain's 'RVSA_MTP' is this package's tap-only class
    net = MODELS.build(m)
    assert isinstance(net, ImageClassifier) and isinstance(net.backbone, mtp_amd.RVSA_MTP_taps) and net.with_neck and net.with_head
    keys = list(net.state_dict())
    assert keys[-2:] == ["head.fc.weight", "head.fc.bias"] and all(k.startswith("backbone.") for k in keys[:-2])
    assert net.head.fc.weight.shape == (10, 768)
    with pytest.raises(ValueError):
        net.extract_feat(torch.zeros(1, 3, 224, 224), stage="head")
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 224, 224), mode="features")


def test_refusals():
    with pytest.raises(NotImplementedError):
        GlobalAveragePooling(dim=1)
    with pytest.raises(NotImplementedError):
        GlobalAveragePooling(dim=3)
    with pytest.raises(ValueError):
        GlobalAveragePooling(dim=4)
    assert GlobalAveragePooling().dim == GlobalAveragePooling(dim=2).dim == 2
    with pytest.raises(TypeError):
        GlobalAveragePooling()(3)
    LinearClsHead(7, 16, loss=dict(type="mmpretrain.CrossEntropyLoss", loss_weight=0.4))
    for loss in (dict(type="LabelSmoothLoss", label_smooth_val=0.1), dict(type="CrossEntropyLoss", use_sigmoid=True), dict(type="CrossEntropyLoss", use_soft=True),
                 dict(type="CrossEntropyLoss", class_weight=[1.0] * 7), dict(type="CrossEntropyLoss", pos_weight=[1.0] * 7),
                 dict(type="CrossEntropyLoss", reduction="sum"), dict(type="mmseg.CrossEntropyLoss")):
        with pytest.raises(NotImplementedError) as e:
            LinearClsHead(7, 16, loss=loss)
        assert repr(loss) in str(e.value)              # the config echoed
    with pytest.raises(NotImplementedError):
        LinearClsHead(7, 16, cal_acc=True)
    with pytest.raises(NotImplementedError):
        LinearClsHead(7, 16, init_cfg=dict(type="Constant", layer="Linear", val=1.0))
    with pytest.raises(ValueError):
        LinearClsHead(7, 16, topk=(1, 8))
    assert LinearClsHead(7, 16, topk=(1, 7)).topk == (1, 7) and LinearClsHead(7, 16, topk=1).topk == (1,)
    head, neck = LinearClsHead(7, 16), GlobalAveragePooling()
    bb = torch.nn.Identity()
    for augments in (dict(type="Mixup", alpha=0.8), [dict(type="Mixup", alpha=0.8), dict(type="CutMix", alpha=1.0)]):
        with pytest.raises(NotImplementedError):
            ImageClassifier(bb, neck, head, train_cfg=dict(augments=augments))
    net = ImageClassifier(bb, neck, head, train_cfg=dict(), data_preprocessor=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True))
    assert list(net.state_dict()) == ["head.fc.weight", "head.fc.bias"]
    with pytest.raises(NotImplementedError):
        Accuracy(thrs=(0.0, 0.5))
    assert Accuracy(thrs=None).thrs is None and Accuracy(thrs=(0.3,)).thrs == 0.3 and Accuracy(topk=5).topk == (5,)
    with pytest.raises(ValueError):
        Accuracy(topk=(5, 1))
    with pytest.raises(ValueError):
        head.forward((torch.zeros(2, 15),))
    with pytest.raises(ValueError):
        head.loss_and_grads(torch.tensor([0, 7]))       # labels outside [0, K): refused on the host
    with pytest.raises(ValueError):
        head.loss_and_grads(torch.tensor([-1, 0]))


def test_fc_init_statistics():
    torch.manual_seed(0)
    head = LinearClsHead(45, 1536)
    w = head.fc.weight.detach().double()
    n = w.numel()                                       # 69120 draws of N(0, 0.01): the mean within 5 sigma / sqrt(n), the std within 5 sigma / sqrt(2 n)
    assert abs(float(w.mean())) < 5 * 0.01 / n ** 0.5 and abs(float(w.std()) - 0.01) < 5 * 0.01 / (2 * n) ** 0.5
    assert float(head.fc.bias.detach().abs().max()) == 0.0 and head.pre_logits((1, 2, 3)) == 3
    assert head.trained_parameter_names() == ["fc.weight", "fc.bias"]
    head.fc.bias.requires_grad_(False)
    assert head.trained_parameter_names() == ["fc.weight"]


def _cpu_hits(scores, labels, topk, thr):
    """the rank rule on the host"""
    hits = [0] * len(topk)
    for s, l in zip(scores.tolist(), labels.tolist()):
        rank = sum(1 for j, v in enumerate(s) if v > s[l] or (v == s[l] and j < l))
        for i, k in enumerate(topk):
            hits[i] += int(rank < k and (thr is None or s[l] > thr))
    return hits + [len(labels)]


def test_accuracy_host_logic(monkeypatch):
    from mtp_amd import ops
    calls = []

    def hits(scores, labels, topk, counters, thr=0.0):      # the kernel's contract on the host
        calls.append((tuple(scores.shape), thr))
        counters += torch.tensor(_cpu_hits(scores, labels, topk, thr))
        return counters
    monkeypatch.setattr(ops, "cls_hits", hits)
    m = Accuracy(topk=(1, 5), thrs=0.0)
    with pytest.raises(RuntimeError):
        m.compute_metrics()
    g = torch.Generator().manual_seed(1)
    want = torch.zeros(3, dtype=torch.int64)
    for n in (1, 7, 64):
        s, l = torch.softmax(torch.randn(n, 10, generator=g), 1), torch.randint(0, 10, (n,), generator=g)
        m.process(s, l)
        want += torch.tensor(_cpu_hits(s, l, (1, 5), 0.0))
    assert m.counters.dtype == torch.int64 and torch.equal(m.counters, want) and len(calls) == 3 and int(want[2]) == 72
    out = m.compute_metrics()
    assert isinstance(out, OrderedDict) and list(out) == ["accuracy/top1", "accuracy/top5"]
    assert out["accuracy/top1"] == float(want[0]) * 100.0 / 72 and out["accuracy/top5"] == float(want[1]) * 100.0 / 72 and isinstance(out["accuracy/top1"], float)
    m.reduce = lambda t: t * 4                              # four ranks with the same counts: the percentages do not move
    assert m.compute_metrics() == out and torch.equal(m.counters, want)
    m.reset()
    assert m.counters is None
    with pytest.raises(ValueError):
        m.process(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64))       # top-5 of 4 classes
    assert Accuracy.counts_to_metrics([3, 7, 8], (1, 5)) == OrderedDict([("accuracy/top1", 37.5), ("accuracy/top5", 87.5)])
    assert Accuracy.counts_to_metrics([1, 3], (2,)) == OrderedDict([("accuracy/top2", 100.0 / 3.0)])
    with pytest.raises(ValueError):
        Accuracy.counts_to_metrics([1, 2], (1, 5))
    # a tie: the label at the higher index of two equal scores ranks second
    s = torch.tensor([[0.4, 0.1, 0.4, 0.1]])
    assert _cpu_hits(s, torch.tensor([2]), (1, 2), 0.0) == [0, 1, 1] and _cpu_hits(s, torch.tensor([0]), (1, 2), 0.0) == [1, 1, 1]


def _check_summary(tensor, gsum, gsamples, tol, n):
    """tests/test_oracle_golden.py's comparison of a (sum, abs-sum) pair and a strided sample"""
    s, v = recipe.summarize(tensor, n)
    assert np.abs(v - gsamples).max() < tol * (np.abs(gsamples).max() + 1e-30)
    assert abs(s[0] - gsum[0]) < 50 * tol * gsum[1] and abs(s[1] - gsum[1]) < tol * gsum[1]


def test_f20_end_to_end_fixture_vs_oracle_backbone_and_torch_head(golden):
    """f20(a) recomputed: oracle.vit_rvsa_oracle.backbone_forward(taps_only=True) and torch operators for the neck, the head and the loss"""
    g = golden("f20_cls_head.npz")
    shapes = recipe.state_shapes(128, 4, 2, 2)
    assert list(shapes) == [str(k) for k in g["a_keys"]]
    p = {k: v.requires_grad_(True) for k, v in recipe.make_params(shapes).items()}
    img = recipe.make_input(2, 224, 224, seed=55).requires_grad_(True)
    w = torch.from_numpy(g["a_fc_weight"]).float().requires_grad_(True)
    b = torch.from_numpy(g["a_fc_bias"]).float().requires_grad_(True)
    assert torch.equal(w.detach().double(), torch.from_numpy(g["a_fc_weight"]))          # f32 values stored as f64
    labels = torch.from_numpy(g["a_labels"])
    feats = O.backbone_forward(img, p, 4, 2, 2, [1, 3], taps_only=True)
    pooled = [F.adaptive_avg_pool2d(f, 1).flatten(1) for f in feats]
    assert rel_err(pooled[0], g["a_pooled0"]) < TOL and rel_err(pooled[1], g["a_pooled1"]) < TOL
    logits = F.linear(pooled[-1], w, b)
    loss = F.cross_entropy(logits, labels)
    scores = torch.softmax(logits.detach(), 1)
    assert rel_err(logits.detach(), g["a_logits"]) < TOL and rel_err(scores, g["a_scores"]) < TOL and abs(float(loss.detach()) - float(g["a_loss"])) < TOL * float(g["a_loss"])
    # the gap condition on the recorded scores, then the hits by the rank rule
    ref = torch.from_numpy(g["a_scores"])
    for anchor in (labels, ref.argmax(1)):
        pa = ref.gather(1, anchor.view(-1, 1))
        ok = (pa - ref).abs() > 1e-4 * torch.maximum(pa.expand_as(ref), ref)
        ok.scatter_(1, anchor.view(-1, 1), True)
        assert bool(ok.all())
    assert _cpu_hits(scores, labels, tuple(g["a_topk"].tolist()), 0.0)[:2] == g["a_hits"].tolist()
    loss.backward()
    assert rel_err(w.grad, g["a_dfc_weight"]) < 5 * TOL and rel_err(b.grad, g["a_dfc_bias"]) < 5 * TOL
    _check_summary(img.grad, g["a_dimg_sum"], g["a_dimg_samples"], 5 * TOL, 2048)
    for n, t in p.items():
        if "a_nograd_" + n in g:
            assert t.grad is None and (n.startswith("fpn") or n.startswith("norm."))
        elif "a_g_" + n in g:
            assert rel_err(t.grad, g["a_g_" + n]) < 5 * TOL, n
        else:
            _check_summary(t.grad, g["a_gs_%s_sum" % n], g["a_gs_%s_samples" % n], 5 * TOL, 1024)
