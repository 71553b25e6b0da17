"""Generate f20_cls_head.npz and f20_cls_configs.json: scene classification (ImageClassifier = backbone -> GlobalAveragePooling -> LinearClsHead with
CrossEntropyLoss, evaluated with Accuracy), everything in float64.

Runs in the development container only (the reference is not on the GPU machine).  The backbone is the reference's own mmpretrain file
(RS_Tasks_Finetune/Scene_Classification/mmpretrain/models/backbones/vit_rvsa_mtp.py through ref_loader.load_reference_cls); mmpretrain itself is not
vendored there, so the neck, the head, the loss and the metric are restated below from the published algorithm and labelled STUB.

  (a) end to end: `RVSA_MTP` with fixture f10's configuration and recipe (embed_dim 128, depth 4, 2 heads, interval 2, out_indices [1, 3], 224 x 224,
      make_params(..., 2023), make_input(2, 224, 224, seed=55), train mode, drop-path 0), then the STUB neck and head with K = 7 classes, labels
      [6, 0] and a seeded N(0, 1) head (the default N(0, 0.01) would put every score gap under any margin).  Recorded: the pooled vectors, logits,
      softmax scores, loss, d fc.weight, d fc.bias, the image-gradient summary and every backbone parameter gradient in f10's g_ / gs_..._sum /
      _samples / nograd_ form, and the top-1 / top-5 hits.
  (b) operator cases: inputs (rounded to bf16-representable values) and float64 results of one pooling and one linear + cross-entropy case; the other
      cases of tests/test_hip_cls_ops.py are regenerated there from seeds with the same torch operators.
  (c) f20_cls_configs.json: the `model` and `val_evaluator` dicts of the eleven Scene_Classification/configs/mtp/*/*.py files as plain JSON settings.

Every case that compares a rank or an arg-max is asserted to satisfy the gap condition: for every sample and every j != label,
|p_label - p_j| > 1e-4 * max(p_label, p_j), and the same around the top-1 class.

    python tests/golden/make_cls_head.py
"""
import contextlib
import glob
import io
import json
import os
import runpy
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import recipe  # noqa: E402
import ref_loader  # noqa: E402

CONFIGS = "/root/reference/RS_Tasks_Finetune/Scene_Classification/configs/mtp"
GAP = 1e-4
K, LABELS, TOPK = 7, [6, 0], (1, 5)


# ---------------------------------------------------------------------------------------------------------------- STUBS
def global_average_pooling(feats):
    """STUB of mmpretrain.models.necks.GlobalAveragePooling(dim=2): AdaptiveAvgPool2d((1, 1)) and a flatten on every map"""
    return tuple(F.adaptive_avg_pool2d(f, 1).flatten(1) for f in feats)


def linear_cls_head(vectors, weight, bias):
    """STUB of mmpretrain.models.heads.LinearClsHead.forward: fc on the last vector"""
    return F.linear(vectors[-1], weight, bias)


def cross_entropy_loss(logits, labels, loss_weight=1.0):
    """STUB of mmpretrain.models.losses.CrossEntropyLoss(use_sigmoid=False, use_soft=False, reduction='mean')"""
    return loss_weight * F.cross_entropy(logits, labels, reduction="mean")


def accuracy_hits(scores, labels, topk, thr=0.0):
    """STUB of mmpretrain.evaluation.Accuracy.calculate for scores: the top max(topk) labels by score; a hit for k when the label is among the first k
    and its score exceeds thr"""
    pred_score, pred_label = scores.topk(max(topk), dim=1)
    correct = pred_label.t().eq(labels.view(1, -1).expand_as(pred_label.t()))
    if thr is not None:
        correct = correct & (pred_score.t() > thr)
    return [int(correct[:k].reshape(-1).sum()) for k in topk]


def bf16_round(t):
    return t.float().bfloat16().double()


def assert_gap(scores, labels):
    """the gap condition: around the label and around the top-1 class, for every sample"""
    for anchor in (labels, scores.argmax(1)):
        pa = scores.gather(1, anchor.view(-1, 1))
        gap = (pa - scores).abs() - GAP * torch.maximum(pa.expand_as(scores), scores)
        gap.scatter_(1, anchor.view(-1, 1), 1.0)
        assert bool((gap > 0).all()), "score gap below %g: choose another seed" % GAP


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def end_to_end(out):
    cls = ref_loader.load_reference_cls()
    net = quiet(cls.RVSA_MTP, img_size=224, patch_size=16, drop_path_rate=0.0, out_indices=[1, 3], embed_dim=128, depth=4, num_heads=2, mlp_ratio=4,
                qkv_bias=True, use_abs_pos_emb=True, interval=2, use_rel_pos_bias=True)
    shapes = recipe.state_shapes(128, 4, 2, 2, 224)
    float_keys = [k for k, v in net.state_dict().items() if v.dtype.is_floating_point]
    assert float_keys == list(shapes.keys())
    msg = net.load_state_dict(recipe.make_params(shapes, 2023), strict=False)
    assert not msg.unexpected_keys and all("relative_position_index" in k for k in msg.missing_keys), msg
    net = net.double().train()
    img = recipe.make_input(2, 224, 224, seed=55).double().requires_grad_(True)
    g = torch.Generator().manual_seed(2020)
    weight = torch.randn(K, 128, generator=g).double().requires_grad_(True)
    bias = torch.randn(K, generator=g).double().requires_grad_(True)
    labels = torch.tensor(LABELS)
    feats = net(img)
    assert isinstance(feats, tuple) and len(feats) == 2 and tuple(feats[1].shape) == (2, 128, 14, 14)
    vectors = global_average_pooling(feats)
    logits = linear_cls_head(vectors, weight, bias)
    loss = cross_entropy_loss(logits, labels)
    loss.backward()
    scores = F.softmax(logits.detach(), dim=1)
    assert_gap(scores, labels)
    out.update({"a_keys": np.array(float_keys), "a_fc_weight": weight, "a_fc_bias": bias, "a_labels": labels, "a_pooled0": vectors[0], "a_pooled1": vectors[1],
                "a_logits": logits, "a_scores": scores, "a_loss": loss, "a_dfc_weight": weight.grad, "a_dfc_bias": bias.grad,
                "a_topk": np.array(TOPK), "a_hits": np.array(accuracy_hits(scores, labels, TOPK))})
    out["a_dimg_sum"], out["a_dimg_samples"] = recipe.summarize(img.grad, 2048)
    for n, p in net.named_parameters():
        if p.grad is None:
            out["a_nograd_" + n] = np.array([1])
        elif p.numel() <= 4096:
            out["a_g_" + n] = p.grad
        else:
            out["a_gs_%s_sum" % n], out["a_gs_%s_samples" % n] = recipe.summarize(p.grad, 1024)


def operator_cases(out):
    g = torch.Generator().manual_seed(20)
    # pooling, the case where nothing is aligned beyond 2 bytes: (N, C, HW) = (2, 5, 49)
    x = bf16_round(torch.randn(2, 5, 49, generator=g))
    dp = bf16_round(torch.randn(2, 5, generator=g))
    out.update({"b_gap_x": x, "b_gap_pooled": x.mean(2), "b_gap_dpooled": dp, "b_gap_dx": (dp / 49).unsqueeze(2).expand(2, 5, 49)})
    # linear + cross-entropy: (N, C, K) = (2, 128, 7), loss_weight 1
    pooled = bf16_round(torch.randn(2, 128, generator=g)).requires_grad_(True)
    w = bf16_round(torch.randn(7, 128, generator=g)).requires_grad_(True)
    b = bf16_round(torch.randn(7, generator=g)).requires_grad_(True)
    labels = torch.tensor([0, 6])
    logits = F.linear(pooled, w, b)
    logits.retain_grad()
    rows = F.cross_entropy(logits, labels, reduction="none")
    loss = cross_entropy_loss(logits, labels)
    loss.backward()
    scores = F.softmax(logits.detach(), dim=1)
    assert_gap(scores, labels)
    out.update({"b_ce_pooled": pooled, "b_ce_w": w, "b_ce_b": b, "b_ce_labels": labels, "b_ce_logits": logits, "b_ce_prob": scores, "b_ce_pred": scores.argmax(1),
                "b_ce_loss_rows": rows, "b_ce_loss": loss, "b_ce_dlogits": logits.grad, "b_ce_dw": w.grad, "b_ce_db": b.grad, "b_ce_dpooled": pooled.grad})


def _plain(v):
    """tuples -> lists: plain JSON settings"""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v


def config_data():
    rec = {}
    for path in sorted(glob.glob(os.path.join(CONFIGS, "*", "*.py"))):
        ns = runpy.run_path(path)
        rec[os.path.relpath(path, CONFIGS)] = {"model": _plain(ns["model"]), "val_evaluator": _plain(ns["val_evaluator"])}
    assert len(rec) == 11
    with open(os.path.join(HERE, "f20_cls_configs.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("f20_cls_configs.json", sorted(rec))


if __name__ == "__main__":
    torch.set_num_threads(8)
    out = {}
    end_to_end(out)
    operator_cases(out)
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "f20_cls_head.npz"), **arrs)
    print("f20_cls_head.npz", {k: v.shape for k, v in arrs.items()})
    config_data()
