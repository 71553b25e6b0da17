"""Generate f16_param_groups.npz: the parameter groups the reference's two layer-decay optimizer constructors build.

Runs in the development container only (the reference is not on the GPU machine).  The constructors
(Multi-Task_Pretrain/mmcv_custom/layer_decay_optimizer_constructor_vit.py and custom_layer_decay_optimizer_constructor.py) are
imported by path with stubs for mmengine.dist / .optim / .registry: a base class that holds base_lr, base_wd and paramwise_cfg, and a
no-op register_module.  Their add_params runs on the reference backbones (built on CPU through ref_loader), each wrapped under the
attribute name the training code gives it ('encoder' in the pretraining script, 'backbone' in the fine-tune frameworks).  Recorded per
model: a digest of the backbone's (name, shape) list (names_digest); per case: the group index of every parameter in that order, and the
groups' names, lr scales and weight decays.

    python tests/golden/make_param_groups.py
"""
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF_CUSTOM = "/root/reference/Multi-Task_Pretrain/mmcv_custom"


class _Constructor:
    """stand-in for mmengine.optim.DefaultOptimWrapperConstructor: what add_params reads"""

    def __init__(self, base_lr, base_wd, paramwise_cfg):
        self.base_lr, self.base_wd, self.paramwise_cfg = base_lr, base_wd, paramwise_cfg


class _Registry:
    def register_module(self, *a, **k):
        return lambda cls: cls


def _install_stubs():
    mm = sys.modules.setdefault("mmengine", types.ModuleType("mmengine"))
    for sub, attrs in (("dist", dict(get_dist_info=lambda: (0, 1))), ("optim", dict(DefaultOptimWrapperConstructor=_Constructor)),
                       ("registry", dict(OPTIM_WRAPPER_CONSTRUCTORS=_Registry()))):
        mod = sys.modules.setdefault("mmengine." + sub, types.ModuleType("mmengine." + sub))
        for k, v in attrs.items():
            setattr(mod, k, v)
        setattr(mm, sub, mod)


def _load(fname, modname):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF_CUSTOM, fname))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


_install_stubs()
import ref_loader  # noqa: E402  (after the stubs: its own mmengine stub is only installed where none exists)

CTOR_VIT = _load("layer_decay_optimizer_constructor_vit.py", "ref_ld_vit").LayerDecayOptimizerConstructor_ViT
CTOR_II = _load("custom_layer_decay_optimizer_constructor.py", "ref_ld_intern").CustomLayerDecayOptimizerConstructor_InternImage
CTORS = {"LayerDecayOptimizerConstructor_ViT": CTOR_VIT, "CustomLayerDecayOptimizerConstructor_InternImage": CTOR_II}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def vit(depth):
    ref = ref_loader.load_reference()

    class A:
        image_size = 224
        use_ckpt = "False"
    return quiet(ref.vit_b_rvsa if depth == 12 else ref.vit_l_rvsa, A)


def internimage(**kw):
    II = ref_loader.load_reference_internimage()
    cfg = dict(core_op="DCNv3_pytorch", channels=192, depths=[5, 5, 24, 5], groups=[12, 24, 48, 96], mlp_ratio=4.0, drop_path_rate=0.2, norm_layer="LN",
               layer_scale=1e-5, offset_scale=2.0, post_norm=True, with_cp=False, out_indices=(0, 1, 2, 3))      # models.py:92-104 (InternImage-XL)
    cfg.update(kw)
    return quiet(II.InternImage, **cfg)


def wrapper(lr, wd, ctor, **paramwise):
    return dict(optimizer=dict(type="AdamW", lr=lr, betas=[0.9, 0.999], weight_decay=wd), constructor=ctor, paramwise_cfg=paramwise)


def names_digest(named):
    """sha256 of the backbone's (name, shape) list -- what tests/test_layer_decay.py compares the repo modules against"""
    return hashlib.sha256("\n".join("%s %s" % (n, list(s)) for n, s in named).encode()).hexdigest()


def run_case(model, prefix, ow):
    wrap = torch.nn.Module()
    setattr(wrap, prefix[:-1], model)
    ctor = CTORS[ow["constructor"]](ow["optimizer"]["lr"], ow["optimizer"]["weight_decay"], dict(ow["paramwise_cfg"]))
    params = []
    quiet(ctor.add_params, params, wrap)
    index = {n: i for i, (n, _) in enumerate(wrap.named_parameters())}
    gid = np.full(len(index), -1, dtype=np.int16)
    for k, g in enumerate(params):
        assert g["lr"] == g["lr_scale"] * ow["optimizer"]["lr"]     # (the recorded scale is what the reference hands torch: lr = scale * base_lr)
        for n in g["param_names"]:
            gid[index[n]] = k
    assert (gid >= 0).all()
    return dict(gid=gid, group_names=np.array([g["group_name"] for g in params]), scales=np.array([g["lr_scale"] for g in params], dtype=np.float64),
                wds=np.array([g["weight_decay"] for g in params], dtype=np.float64))


VIT = "LayerDecayOptimizerConstructor_ViT"
II = "CustomLayerDecayOptimizerConstructor_InternImage"
II_XL = dict(num_layers=39, layer_decay_rate=0.94, depths=[5, 5, 24, 5])
# InternImage-H-style switches (level-2 post-norms after blocks 5 / 11 / 17 / 23, res-post-norms, center feature scale) at a small width
II_L2 = dict(channels=32, groups=[2, 4, 8, 16], layer_scale=None, post_norm=False, res_post_norm=True, level2_post_norm=True,
             level2_post_norm_block_ids=[5, 11, 17, 23], dw_kernel_size=5, center_feature_scale=True, drop_path_rate=0.0)


CASES = {     # case -> (model, prefix, optim_wrapper)
    "vit_b_backbone": ("vit_b", "backbone.", wrapper(6e-5, 0.05, VIT, num_layers=12, layer_decay_rate=0.9)),
    "vit_l_backbone": ("vit_l", "backbone.", wrapper(6e-5, 0.05, VIT, num_layers=24, layer_decay_rate=0.9)),
    "vit_l_encoder": ("vit_l", "encoder.", wrapper(6e-5, 0.05, VIT, num_layers=24, layer_decay_rate=0.9)),
    "internimage_xl_encoder": ("internimage_xl", "encoder.", wrapper(2e-5, 0.05, II, **II_XL)),
    "internimage_xl_backbone": ("internimage_xl", "backbone.", wrapper(2e-5, 0.05, II, **II_XL)),
    "internimage_l2postnorm_encoder": ("internimage_l2postnorm", "encoder.", wrapper(2e-5, 0.05, II, **II_XL)),
    "internimage_l2postnorm_encoder_small_lr": ("internimage_l2postnorm", "encoder.", wrapper(2e-5, 0.05, II, backbone_small_lr=True, **II_XL)),
    "internimage_l2postnorm_backbone": ("internimage_l2postnorm", "backbone.", wrapper(2e-5, 0.05, II, offset_lr_scale=0.5, **II_XL)),
}
MODELS = {"vit_b": lambda: vit(12), "vit_l": lambda: vit(24), "internimage_xl": internimage, "internimage_l2postnorm": lambda: internimage(**II_L2)}


def main():
    torch.manual_seed(0)
    out = {"cases": np.array(json.dumps({k: dict(model=m, prefix=p, optim_wrapper=ow) for k, (m, p, ow) in CASES.items()}))}
    for model, make in MODELS.items():
        m = make()
        out[model + ".names_digest"] = np.array(names_digest([(n, tuple(p.shape)) for n, p in m.named_parameters()]))
        for case, (mk, prefix, ow) in CASES.items():
            if mk == model:
                for k, v in run_case(m, prefix, ow).items():
                    out[case + "." + k] = v
        del m
    path = os.path.join(HERE, "f16_param_groups.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: len(out[k + ".group_names"]) for k in CASES})


if __name__ == "__main__":
    main()
