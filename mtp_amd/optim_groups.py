"""Layer-wise learning-rate decay: the parameter groups of the reference's two optimizer constructors.

Restates `add_params` of
  * LayerDecayOptimizerConstructor_ViT (mmcv_custom/layer_decay_optimizer_constructor_vit.py:7-79), and
  * CustomLayerDecayOptimizerConstructor_InternImage (mmcv_custom/custom_layer_decay_optimizer_constructor.py:17-152)
for the mmengine-style `optim_wrapper` dicts the reference's scripts and configs write, quirks included:
  * num_layers is the config's value + 2 (never the model depth);
  * the layer rules test the FULL parameter name: the ViT rule looks for `backbone.*`, the InternImage rule for `encoder.*`
    (+ `level_embeds` anywhere), so under the other prefix every parameter falls to layer num_layers - 1 (scale 1);
  * InternImage: `levels.i.post_norms.k` takes its layer id from k; a level's downsample and closing norm take 1 + sum(depths[:i+1])
    (level 3 the same as level 2); `sampling_offsets` / `reference_points` under a name containing `backbone` form groups of their own
    scaled by `offset_lr_scale`; `backbone_small_lr` multiplies every scale below 1 by 0.1; `dino_head` as in :105-107.
The groups come back in first-seen order as [(group_name, lr_scale, weight_decay, [names])] -- the shape of
mtp_amd.parallel.reference_param_groups -- with the names as given (the prefix only feeds the rules)."""
import copy

# main_pretrain.py:424-474: the optimizer of each pretraining backbone
PRETRAIN_OPTIM_WRAPPERS = {
    "vit_b": dict(optimizer=dict(type="AdamW", lr=6e-5, betas=(0.9, 0.999), weight_decay=0.05),
                  constructor="LayerDecayOptimizerConstructor_ViT", paramwise_cfg=dict(num_layers=12, layer_decay_rate=0.9)),
    "vit_l": dict(optimizer=dict(type="AdamW", lr=6e-5, betas=(0.9, 0.999), weight_decay=0.05),
                  constructor="LayerDecayOptimizerConstructor_ViT", paramwise_cfg=dict(num_layers=24, layer_decay_rate=0.9)),
    "internimage_xl": dict(optimizer=dict(type="AdamW", lr=2e-5, betas=(0.9, 0.999), weight_decay=0.05),
                           constructor="CustomLayerDecayOptimizerConstructor_InternImage",
                           paramwise_cfg=dict(num_layers=39, layer_decay_rate=0.94, depths=[5, 5, 24, 5])),
}

CONSTRUCTORS = ("LayerDecayOptimizerConstructor_ViT", "CustomLayerDecayOptimizerConstructor_InternImage")


def pretrain_optim_wrapper(backbone):
    """a fresh copy of the reference's optim_wrapper for 'vit_b' / 'vit_l' / 'internimage_xl'"""
    if backbone not in PRETRAIN_OPTIM_WRAPPERS:
        raise KeyError("no pretraining optimizer preset %r (have %s)" % (backbone, ", ".join(sorted(PRETRAIN_OPTIM_WRAPPERS))))
    return copy.deepcopy(PRETRAIN_OPTIM_WRAPPERS[backbone])


def optimizer_hyper(optim_wrapper):
    """(lr, betas, weight_decay) of the wrapper's AdamW"""
    opt = optim_wrapper.get("optimizer", {})
    if opt.get("type", "AdamW") != "AdamW":
        raise ValueError("the fused optimizer is AdamW; the optim_wrapper asks for %r" % (opt.get("type"),))
    return float(opt["lr"]), tuple(float(b) for b in opt.get("betas", (0.9, 0.999))), float(opt.get("weight_decay", 0.0))


def _vit_layer(name, num_max_layer):
    """get_num_layer_for_vit (layer_decay_optimizer_constructor_vit.py:7-16)"""
    if name in ("backbone.cls_token", "backbone.mask_token", "backbone.pos_embed"):
        return 0
    if name.startswith("backbone.patch_embed"):
        return 0
    if name.startswith("backbone.blocks"):
        return int(name.split(".")[2]) + 1
    return num_max_layer - 1


def _intern_layer(name, num_max_layer, depths):
    """get_num_layer_for_swin (custom_layer_decay_optimizer_constructor.py:17-59)"""
    if name.startswith(("encoder.patch_embed", "decode_head.mask_embed", "decode_head.cls_embed", "decode_head.level_embed",
                        "decode_head.query_embed", "decode_head.query_feat")):
        return 0
    if name.startswith("encoder.cb_modules.0.patch_embed"):
        return 0
    if "level_embeds" in name:
        return 0
    if name.startswith("encoder.layers") or name.startswith("encoder.levels"):
        parts = name.split(".")
        stage = int(parts[2])
        if parts[3] not in ("downsample", "norm"):
            return int(parts[4]) + 1 + sum(depths[:min(stage, 3)])
        return 1 + sum(depths[:min(stage, 2) + 1])
    return num_max_layer - 1


def layer_decay_param_groups(named, optim_wrapper, prefix="encoder."):
    """named: (name, shape) pairs, or (name, tensor) -- tensors with requires_grad=False are skipped, as the constructors do.
    optim_wrapper: dict(optimizer=dict(type='AdamW', lr, betas, weight_decay), constructor=<one of CONSTRUCTORS>, paramwise_cfg=dict(...)).
    prefix: what the model that the constructor sees calls the backbone ('encoder.' in the pretraining script, 'backbone.' in the
    fine-tune frameworks).  Returns [(group_name, lr_scale, weight_decay, [names])] in first-seen order."""
    ctor = optim_wrapper.get("constructor")
    if ctor not in CONSTRUCTORS:
        raise ValueError("optim_wrapper constructor must be one of %s, got %r" % (", ".join(CONSTRUCTORS), ctor))
    cfg = optim_wrapper.get("paramwise_cfg") or {}
    _, _, weight_decay = optimizer_hyper(optim_wrapper)
    num_layers = cfg.get("num_layers") + 2
    rate = cfg.get("layer_decay_rate")
    vit = ctor == CONSTRUCTORS[0]
    depths = cfg.get("depths")
    backbone_small_lr = cfg.get("backbone_small_lr", False)
    dino_head = cfg.get("dino_head", False)
    offset_lr_scale = cfg.get("offset_lr_scale", 1.0)
    groups, order = {}, []
    for n, p in named:
        if getattr(p, "requires_grad", True) is False:
            continue
        shape = tuple(p.shape) if hasattr(p, "shape") else tuple(p)
        full = prefix + n
        if vit:
            nd = len(shape) == 1 or full.endswith(".bias") or "pos_embed" in full
        else:
            nd = len(shape) == 1 or full.endswith(".bias") or "relative_position" in full or "norm" in full or "sampling_offsets" in full
        kind, wd = ("no_decay", 0.0) if nd else ("decay", weight_decay)
        if vit:
            layer_id = _vit_layer(full, num_layers)
            key = "layer_%d_%s" % (layer_id, kind)
        else:
            layer_id = _intern_layer(full, num_layers, depths)
            offs = "sampling_offsets" in full or "reference_points" in full
            if layer_id == num_layers - 1 and dino_head and offs:
                key = "layer_%d_%s_0.1x" % (layer_id, kind)
            elif offs and "backbone" in full:
                key = "layer_%d_%s_offset_lr_scale" % (layer_id, kind)
            else:
                key = "layer_%d_%s" % (layer_id, kind)
        if key not in groups:
            scale = rate ** (num_layers - layer_id - 1)
            if not vit:
                if scale < 1 and backbone_small_lr is True:
                    scale = scale * 0.1
                if "0.1x" in key:
                    scale = scale * 0.1
                if "offset_lr_scale" in key:
                    scale = scale * offset_lr_scale
            groups[key] = (key, scale, wd, [])
            order.append(key)
        groups[key][3].append(n)
    return [groups[k] for k in order]
