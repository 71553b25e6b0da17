"""GPU: the scene-classification modules -- GlobalAveragePooling, LinearClsHead, ImageClassifier, Accuracy -- every workspace out of a guard.Arena.
  * the autograd surface (`loss(...).backward()`) and the fast path (`loss_and_grads`) run the same kernels: loss, parameter gradients and the last
    map's gradient are bit-identical, f32 and bf16 maps; the other maps get None;
  * predict in eval mode against the float64 softmax (arg-max exact under the gap condition), the training flag restored;
  * fixture f20(a) (tests/golden/make_cls_head.py: the reference's own mmpretrain backbone file, then the restated neck / head / loss, float64) on the
    device with RVSA_MTP_taps at fixture f10's tolerances (tests/test_hip_backbone.py::test_tap_only_finetune_variant_vs_reference): fp32 1e-3
    everywhere; bf16 4e-2 forward, 0.35 gradients, 0.6 for the sampling heads; norm.* / fpn* without a gradient; Accuracy reproduces the hits."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import guard
import mtp_amd
from conftest import ROOT, record_parity, rel_err
from mtp_amd import Accuracy, GlobalAveragePooling, ImageClassifier, LinearClsHead, ops

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import recipe  # noqa: E402

pytestmark = pytest.mark.gpu
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64


@pytest.fixture(autouse=True)
def arena(monkeypatch):
    a = guard.Arena("cuda")
    monkeypatch.setattr(ops, "_scratch", a.scratch)
    yield a
    torch.cuda.synchronize()
    try:
        a.check()
    finally:
        a.close()


class _Taps(nn.Module):
    """two maps from torch's own convolutions: plumbing in front of the modules under test"""

    def __init__(self, dtype):
        super().__init__()
        self.c0, self.c1, self.dtype = nn.Conv2d(3, 8, 3, 4), nn.Conv2d(8, 16, 3, 2), dtype

    def forward(self, x):
        f0 = self.c0(x)
        return f0.to(self.dtype), self.c1(f0).to(self.dtype)


def _classifier(dtype, seed=0):
    torch.manual_seed(seed)
    net = ImageClassifier(_Taps(dtype), dict(type="GlobalAveragePooling"), dict(type="LinearClsHead", num_classes=5, in_channels=16,
                                                                               loss=dict(type="CrossEntropyLoss", loss_weight=0.7), topk=(1, 5)))
    with torch.no_grad():
        net.head.fc.weight.normal_(0.0, 1.0)
        net.head.fc.bias.normal_(0.0, 1.0)
    return net.cuda().train()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_autograd_surface_and_fast_path_are_bit_identical(dtype):
    net = _classifier(dtype)
    img = torch.randn(3, 3, 61, 45, generator=torch.Generator().manual_seed(1)).cuda()      # maps 15 x 11 and 7 x 5: odd row lengths
    labels = torch.tensor([4, 0, 2]).cuda()
    feats = [f.detach().requires_grad_(True) for f in net.extract_feat(img, stage="backbone")]
    assert feats[1].shape == (3, 16, 7, 5) and feats[1].dtype == dtype
    vecs = net.neck(tuple(feats))
    assert isinstance(vecs, tuple) and [tuple(v.shape) for v in vecs] == [(3, 8), (3, 16)] and all(v.dtype == F32 for v in vecs)
    assert torch.is_tensor(net.neck(feats[0])) and not list(net.neck.parameters())
    loss = net.head.loss(vecs, labels)
    assert list(loss) == ["loss"]
    loss["loss"].backward()
    want = (loss["loss"].detach().clone(), net.head.fc.weight.grad.clone(), net.head.fc.bias.grad.clone(), feats[1].grad.clone())
    assert feats[0].grad is None and want[3].dtype == dtype and want[3].shape == feats[1].shape
    # the reference, float64 on the same maps
    fr = feats[1].detach().double().requires_grad_(True)
    w, b = net.head.fc.weight.detach().double().requires_grad_(True), net.head.fc.bias.detach().double().requires_grad_(True)
    ref = 0.7 * nn.functional.cross_entropy(nn.functional.linear(fr.mean((2, 3)), w, b), labels)
    ref.backward()
    tol = 1e-5 if dtype == F32 else 2.0 ** -8
    assert abs(float(want[0]) - float(ref.detach())) < 1e-5 * float(ref.detach()) and rel_err(want[1], w.grad) < 1e-5 and rel_err(want[2], b.grad) < 1e-5
    assert rel_err(want[3].float(), fr.grad) < tol
    # the fast path: no autograd, gradients accumulated into .grad
    net.head.zero_grad(set_to_none=True)
    with torch.no_grad():
        l2, dfeats = net.head.loss_and_grads(labels)([f.detach() for f in feats])
    assert dfeats[0] is None and len(dfeats) == 2 and dfeats[1].dtype == dtype
    assert torch.equal(l2, want[0]) and torch.equal(net.head.fc.weight.grad, want[1]) and torch.equal(net.head.fc.bias.grad, want[2])
    assert torch.equal(dfeats[1], want[3])
    net.head.loss_and_grads(labels)([f.detach() for f in feats])          # a second call accumulates
    assert rel_err(net.head.fc.weight.grad, 2 * want[1]) < 1e-6 and rel_err(net.head.fc.bias.grad, 2 * want[2]) < 1e-6
    # the whole classifier through autograd: forward(mode='loss') reaches the backbone's parameters
    net.zero_grad(set_to_none=True)
    out = net(img, labels, mode="loss")
    out["loss"].backward()
    assert rel_err(out["loss"].detach(), want[0]) < 1e-5 and rel_err(net.head.fc.weight.grad, want[1]) < 1e-4      # (the convolutions ran again)
    assert net.backbone.c0.weight.grad is not None and float(net.backbone.c1.weight.grad.abs().max()) > 0


def test_predict_in_eval_mode_and_tensor_mode():
    net = _classifier(F32, 3)
    img = torch.randn(4, 3, 61, 45, generator=torch.Generator().manual_seed(2)).cuda()
    logits = net(img)                                   # mode='tensor'
    assert logits.shape == (4, 5) and logits.requires_grad
    out = net(img, mode="predict")
    assert net.training and net.head.training and list(out) == ["pred_score", "pred_label"]
    assert out["pred_score"].shape == (4, 5) and out["pred_label"].dtype == I64 and not out["pred_score"].requires_grad
    f = net.extract_feat(img, stage="pre_logits")
    assert f.shape == (4, 16)
    ref = torch.softmax(nn.functional.linear(f.detach().double(), net.head.fc.weight.detach().double(), net.head.fc.bias.detach().double()), 1).cpu()
    top = ref.argmax(1)
    pa = ref.gather(1, top.view(-1, 1))
    ok = (pa - ref).abs() > 1e-4 * torch.maximum(pa.expand_as(ref), ref)
    ok.scatter_(1, top.view(-1, 1), True)
    assert bool(ok.all())                               # the gap condition around the top-1 class, every sample
    assert rel_err(out["pred_score"].cpu(), ref) < 1e-5 and torch.equal(out["pred_label"].cpu(), top)
    assert rel_err(torch.softmax(logits.detach(), 1).cpu(), ref) < 1e-5


def _check_summary(tensor, gsum, gsamples, tol, n, what):
    """tests/test_hip_backbone.py's: max-abs error relative to the largest sample, plus relative L2 over the samples"""
    s, v = recipe.summarize(tensor.float().cpu(), n)
    err = np.abs(v - gsamples).max() / (np.abs(gsamples).max() + 1e-30)
    l2 = np.linalg.norm(v - gsamples) / (np.linalg.norm(gsamples) + 1e-30)
    assert err < tol and l2 < tol, (what, float(err), float(l2))
    assert abs(s[1] - gsum[1]) < tol * gsum[1], what
    return float(err)


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 4e-2)])
def test_f20_end_to_end_on_the_device(golden, precision, tol):
    g = golden("f20_cls_head.npz")
    bb = mtp_amd.RVSA_MTP_taps(img_size=224, embed_dim=128, depth=4, num_heads=2, interval=2, qkv_bias=True, use_abs_pos_emb=True, out_indices=[1, 3],
                               precision=precision, feature_dtype=F32, frozen_stages=-1)
    assert [k for k, v in bb.state_dict().items() if v.dtype.is_floating_point] == [str(k) for k in g["a_keys"]]
    bb.load_state_dict(recipe.make_params(recipe.state_shapes(128, 4, 2, 2)), strict=False)
    net = ImageClassifier(bb, GlobalAveragePooling(), LinearClsHead(7, 128, topk=(1, 5)))
    net.head.load_state_dict({"fc.weight": torch.from_numpy(g["a_fc_weight"]).float(), "fc.bias": torch.from_numpy(g["a_fc_bias"]).float()})
    net = net.cuda().train()
    img = recipe.make_input(2, 224, 224, seed=55).cuda().requires_grad_(True)
    labels = torch.from_numpy(g["a_labels"]).cuda()
    vecs = net.extract_feat(img, stage="neck")
    assert len(vecs) == 2 and rel_err(vecs[0].cpu(), g["a_pooled0"]) < tol and rel_err(vecs[1].cpu(), g["a_pooled1"]) < tol
    loss = net.head.loss(vecs, labels)["loss"]
    pred = net.head.predict(vecs)
    group = "cls_f20_" + precision
    for name, got, want in (("logits", net.head(vecs).detach(), g["a_logits"]), ("scores", pred["pred_score"], g["a_scores"]), ("loss", loss.detach(), g["a_loss"])):
        v = rel_err(got.cpu(), want)
        record_parity(group, name, v)
        assert v < tol, (name, v)
    metric = Accuracy(topk=tuple(int(k) for k in g["a_topk"]))
    assert metric.counters is None
    metric.process(pred["pred_score"], labels)
    assert metric.counters.cpu().tolist() == g["a_hits"].tolist() + [2]
    assert metric.compute_metrics() == {"accuracy/top1": 100.0 * g["a_hits"][0] / 2, "accuracy/top5": 100.0 * g["a_hits"][1] / 2}
    loss.backward()
    gt = tol if precision == "fp32" else 0.35
    for name, got, want in (("fc.weight", net.head.fc.weight.grad, g["a_dfc_weight"]), ("fc.bias", net.head.fc.bias.grad, g["a_dfc_bias"])):
        v = rel_err(got.cpu(), want)
        record_parity(group, "d " + name, v)
        assert v < gt, (name, v)
    _check_summary(img.grad, g["a_dimg_sum"], g["a_dimg_samples"], gt, 2048, "dimg")
    for n, p in bb.named_parameters():
        lim = 0.6 if (precision == "bf16" and "sampling" in n) else gt
        if "a_nograd_" + n in g:
            assert p.grad is None and (n.startswith("norm.") or n.startswith("fpn")), n
        elif "a_g_" + n in g:
            assert rel_err(p.grad.cpu(), g["a_g_" + n]) < lim, n
        else:
            assert _check_summary(p.grad, g["a_gs_%s_sum" % n], g["a_gs_%s_samples" % n], gt, 1024, n) < lim, n
