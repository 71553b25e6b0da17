"""Float64 reference of the flat-buffer optimizer step (csrc/optimizer.hip) and the buffer layouts its entry points take.

Plain helper module: no fixtures, no plugin, CPU only (tests/test_optim_ref_host.py checks it against torch.optim.AdamW; tests/test_hip_step_edges.py
holds the HIP kernels to it).

* `adamw_ref` / `adamw_parts`: one AdamW step with gradient clipping over a flat buffer, every operation in float64 on the values it is given.
* `layout`: flat offsets (every parameter padded to 64 elements, as FlatParams pads them) and the (R, C, tile0) of the mtp_wimg_desc rows of a list of
  (shape, has_w, has_wt, f32_out); `wimg_descs` fills the `_lib.WimgDesc` table from it (the logic of test_hip_layer_decay._descs).
* `exact_ints`: f32 values in {-1, 0, 1}, whose squares and partial sums are integers <= n: exact in f32 in any order of summation.
"""
import torch

PAD = 64


def _f64(x):
    """the values of x (tensor or sequence of Python / f32 numbers) as a float64 tensor: an f32 tensor keeps its f32 VALUES"""
    return x.detach().cpu().double() if isinstance(x, torch.Tensor) else torch.tensor([float(v) for v in x], dtype=torch.float64)


def clip_scale(sqn, max_norm, grad_scale):
    """optimizer.hip:clipped_grad_scale in float64: grad_scale, times clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)) when the squared norm
    of the UNSCALED gradients is given"""
    gs = float(grad_scale)
    if sqn is not None:
        total = float(sqn) ** 0.5 * gs
        coef = float(max_norm) / (total + 1e-6)
        gs *= coef if coef < 1.0 else 1.0
    return gs


def adamw_parts(p, g, m, v, seg_start, seg_wd, seg_lr, hyper, sqn, max_norm, grad_scale):
    """one step over the flat buffers p / g / m / v (n elements; segment s = [seg_start[s], seg_start[s + 1]) with weight decay seg_wd[s] and, unless
    seg_lr is None, lr = hyper[0] * seg_lr[s]); hyper = (lr, beta1, beta2, eps, 1 - beta1^t, 1 - beta2^t).  Everything in float64 on the input values:
    the constants the kernel forms in f32 (lr * wd, 1 - lr * wd, lr / bc1, 1 / sqrt(bc2)) are formed here in f64 from the hyper values as given.
    Returns a dict: the new p / m / v, and the terms the error bounds are made of (ge = the scaled gradient, decayed = p (1 - lr wd), update = what is
    subtracted from it, and the two addends of each moment)."""
    p, g, m, v = (_f64(t).reshape(-1) for t in (p, g, m, v))
    n = p.numel()
    lr0, b1, b2, eps, bc1, bc2 = (float(x) for x in _f64(hyper))
    start = [int(s) for s in (seg_start.tolist() if isinstance(seg_start, torch.Tensor) else seg_start)]
    wd = _f64(seg_wd)
    sc = torch.ones(len(start), dtype=torch.float64) if seg_lr is None else _f64(seg_lr)
    assert start[0] == 0 and all(a < b for a, b in zip(start, start[1:])) and start[-1] < n and len(start) == wd.numel() == sc.numel()
    count = torch.tensor([b - a for a, b in zip(start, start[1:] + [n])])
    lr = torch.repeat_interleave(lr0 * sc, count)
    decay = 1.0 - lr * torch.repeat_interleave(wd, count)
    step = lr / bc1
    rbc2 = bc2 ** -0.5
    gs = clip_scale(None if sqn is None else (sqn.item() if isinstance(sqn, torch.Tensor) else sqn), max_norm, grad_scale)
    ge = g * gs
    m1, m2 = b1 * m, (1.0 - b1) * ge
    v1, v2 = b2 * v, (1.0 - b2) * ge * ge
    mn, vn = m1 + m2, v1 + v2
    decayed = p * decay
    update = step * mn / (vn.sqrt() * rbc2 + eps)
    return dict(p=decayed - update, m=mn, v=vn, ge=ge, decayed=decayed, update=update, m_terms=m1.abs() + m2.abs(), v_terms=v1.abs() + v2.abs(), gs=gs)


def adamw_ref(p, g, m, v, seg_start, seg_wd, seg_lr, hyper, sqn, max_norm, grad_scale):
    """(p, m, v) after one step, float64: optimizer.hip:adamw_elem with clipped_grad_scale, i.e. torch.optim.AdamW after clip_grad_norm_ (see adamw_parts)"""
    r = adamw_parts(p, g, m, v, seg_start, seg_wd, seg_lr, hyper, sqn, max_norm, grad_scale)
    return r["p"], r["m"], r["v"]


# ------------------------------------------------------------------------------------------------ layouts
def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def layout(shapes):
    """shapes: [(shape, has_w, has_wt, f32_out)] -> (segments, total): one dict per parameter with its flat offset `off` (multiples of 64), `numel`, `padded`,
    the descriptor's matrix (R, C) -- the parameter itself when it is 2-D, rows of 64 INCLUDING the padding when it is 1-D -- its first tile `tile0` and its tile
    count; total = the length of the flat buffers"""
    segs, off, tile0 = [], 0, 0
    for shape, has_w, has_wt, f32_out in shapes:
        shape = tuple(int(d) for d in shape)
        numel = _numel(shape)
        padded = (numel + PAD - 1) // PAD * PAD
        assert len(shape) in (1, 2) and (len(shape) == 2 or not (has_w or has_wt))
        R, Cc = shape if len(shape) == 2 else (padded // PAD, PAD)
        tiles = ((R + 63) // 64) * ((Cc + 63) // 64)
        segs.append(dict(shape=shape, off=off, numel=numel, padded=padded, R=R, C=Cc, tile0=tile0, tiles=tiles, has_w=bool(has_w), has_wt=bool(has_wt),
                         f32_out=bool(f32_out)))
        off += padded
        tile0 += tiles
    return segs, off


def total_tiles(segs):
    return segs[-1]["tile0"] + segs[-1]["tiles"]


def wimg_descs(segs, p, images, wd):
    """the _lib.WimgDesc table (a ctypes array) of `segs` over the flat parameter buffer p: images[i] = (w or None, wt or None), wd[i] = the weight decay"""
    from mtp_amd import _lib
    arr = (_lib.WimgDesc * len(segs))()
    for i, sg in enumerate(segs):
        d = arr[i]
        w, wt = images[i] if images[i] is not None else (None, None)
        d.src = p.data_ptr() + 4 * sg["off"]
        d.w, d.wt = (w.data_ptr() if w is not None else None), (wt.data_ptr() if wt is not None else None)
        d.R, d.C, d.tile0, d.f32_out, d.wd = sg["R"], sg["C"], sg["tile0"], int(sg["f32_out"]), float(wd[i])
    return arr


def table_bytes(arr):
    """a ctypes descriptor table as a uint8 CPU tensor (to be copied to the device)"""
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)


# the seam layout of tests/test_hip_step_edges.py: R and C out of {1, 4, 8, 12, 60, 64, 68, 72, 136} (one element, the 4- and 8-element store widths, one
# column group short of / exactly / one and two groups past the 64 tile, two tiles and a ragged third), every image combination, f32 and activation-dtype
# images, 1-D parameters of 1, 4, 63, 64, 65 elements between them, and (10, 6): off every vector width, element-wise whatever the dtype.
# With bf16 images a matrix is on the vector path when C % 8 == 0 (and R % 8 == 0 if it has a transposed image); with f32 images (f32_out, or f32
# activations) C % 4 / R % 4; without images C % 4.  C % 8 == 4 on the vector path -- (12, 60) f32, (72, 68), (60, 12), (8, 12), (4, 4) -- is where the last
# column group of a row holds one quad, not two.
SEAM_SHAPES = [
    ((64, 64), True, True, False), ((1,), False, False, False), ((8, 136), True, True, False), ((4,), False, False, False), ((136, 8), True, True, True),
    ((63,), False, False, False), ((12, 60), True, False, False), ((64,), False, False, False), ((68, 72), True, True, False), ((65,), False, False, False),
    ((72, 68), False, True, True), ((4, 4), True, True, True), ((1, 64), True, False, False), ((64, 1), False, True, False), ((60, 12), False, False, False),
    ((10, 6), True, True, False), ((136, 136), True, True, False), ((8, 8), False, True, False), ((1, 1), True, True, False), ((72, 8), True, False, True),
    ((8, 12), True, True, True), ((12, 4), False, False, False), ((60, 72), True, False, False),
]
# every size exact_ints is asked for by the GPU tests: the plain squared norm, the base buffer of the segment tables, the row reductions
SQNORM_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 2048 + 5]
SEGMENT_BASE = 3 * 65536 + 4097 * 8 + 4096
REDUCE_SIZES = [rows * cols for rows in (1, 2, 255, 257) for cols in (4, 12, 260, 1, 15, 64)]


# ------------------------------------------------------------------------------------------------ exact inputs
def exact_ints(n, seed=0):
    """n f32 values in {-1, 0, 1}: every square and every partial sum of them or of their squares, in any order, is an integer of magnitude <= n, hence
    exact in f32 for n < 2^24 -- a sum kernel must return the integer itself, whatever its order of accumulation"""
    assert 0 < n < 2 ** 24
    g = torch.Generator().manual_seed(1000003 * seed + n)
    return (torch.randint(0, 3, (n,), generator=g) - 1).float()
