"""Golden vectors of the validation inputs (unidepth_amd/testprep.py, csrc/testprep.hip): the reference's own test-time ContextCrop
(unidepth/datasets/pipelines/transforms.py, torch on the CPU) and its Pinhole / BatchCamera on seeded inputs -> tests/golden/testprep.npz.

    python tools/make_golden_testprep.py          (needs the reference tree; only its outputs are written)

This module also holds what the tests share: WINDOW_CASES / PREP_CASES / GEOMETRY_SIZES with case_inputs(name) (seeded CPU
torch.Generator inputs, uniform draws only, the same bits on every machine), an independent numpy restatement of ud_resize_aa
(include/unidepth_hip.h UdResizeAA) -- restate(..., dtype=np.float32) rounds every operation separately in fp32, the kernel's
definition, reproduced bit for bit; dtype=np.float64 is the same expression in fp64, the value the tolerances are measured from -- and
torch_composition(), what a user writes without the kernel (slice, F.pad, F.interpolate(antialias=True), round, clamp, /255,
normalise, per plane).

torchvision is not installed where the golden file is written.  reference_modules() therefore registers a small
torchvision.transforms.v2.functional stand-in in sys.modules before it loads transforms.py by file path: resize = F.interpolate on the
float cast (then round and clamp for uint8; the nearest rule for NEAREST), pad = zero F.pad, InterpolationMode.  So the FILTER
ARITHMETIC in the golden file is ATen's CPU _upsample_bicubic2d_aa / _upsample_bilinear2d_aa (fp32), and the torchvision CASTING RULE
(uint8 -> float, interpolate, round, clamp to [0, 255], cast back) is restated from memory of torchvision's source, not executed from
it.  The network shape, window, paddings, zoom and camera come from the reference's own code with its own Pinhole / BatchCamera.
Nothing from the reference is imported at module import time."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "testprep.npz")
REF_TRANSFORMS = os.path.join("unidepth", "datasets", "pipelines", "transforms.py")

FILTERS = ("bicubic", "bilinear")
MEAN = (0.485, 0.456, 0.406)                       # the reference's ImageNet statistics (datasets/base_dataset.py)
STD = (0.229, 0.224, 0.225)

# name -> ((h, w) source, window (top, left, height, width) or None for the whole image, (Hn, Wn) destination)
WINDOW_CASES = {
    "w37x53_pad_tb": ((37, 53), (-4, 0, 45, 53), (28, 42)),
    "w45x60_pad_lr": ((45, 60), (0, -7, 45, 74), (42, 70)),
    "w97x131_cut": ((97, 131), (5, 9, 80, 100), (28, 42)),
    "w30x40_up": ((30, 40), (-3, -2, 36, 44), (56, 70)),
    "w9x11_full": ((9, 11), None, (14, 14)),
    "w20x31_full": ((20, 31), None, (14, 28)),
    "w50x3_beside": ((50, 3), (0, -30, 50, 63), (28, 28)),
}

# shape_constraints: the released V2 configs (configs/config_v2_*.json), the V1 training config (configs/train_v1_vitl14.json: its
# pixels_min is above its pixels_max, so every image gets pixels_min), and a small set for the cases whose pixels are stored
CONSTRAINTS = {
    "v2": dict(ratio_bounds=[0.5, 2.5], pixels_max=600000, pixels_min=200000, height_min=15, width_min=15, shape_mult=14, sample=True),
    "v1train": dict(ratio_bounds=[0.66, 2.0], pixels_max=200000, pixels_min=400000, height_min=15, width_min=15, shape_mult=14, sample=True),
    "small": dict(ratio_bounds=[0.5, 2.5], pixels_max=6000, pixels_min=2000, shape_mult=14, sample=True),
}
GEOMETRY_SIZES = [(480, 640), (375, 1242), (1242, 375), (518, 518), (100, 1000), (37, 53)]
GEOMETRY_SETS = ("v2", "v1train")
IMAGE_SHAPE = (518, 518)                           # the configs' data.image_shape; replaced by test_closest_shape when sample is true

# name -> (B, (h, w), constraints, mask given): ContextCrop on pixels, stored in the golden file
PREP_CASES = {
    "p37x53": (2, (37, 53), "small", False),
    "p97x131": (1, (97, 131), "small", True),
    "p60x300_wide": (1, (60, 300), "small", True),
    "p120x41_tall": (2, (120, 41), "small", False),
}


def _seed(name):
    return 5200 + sorted(list(WINDOW_CASES) + list(PREP_CASES)).index(name)


def case_inputs(name):
    """window case: (src uint8 [B,3,h,w], src fp32 [B,3,h,w] in [-64, 320), window, (Hn, Wn));
    prep case: (image uint8 [B,3,h,w], validity mask uint8 [B,1,h,w] or None, K fp32 [B,3,3], constraints dict)."""
    g = torch.Generator().manual_seed(_seed(name))
    if name in WINDOW_CASES:
        (h, w), win, size = WINDOW_CASES[name]
        B = 1 if size[0] * size[1] >= 1000 else 4                                # at least ~3000 destination pixels per case
        u8 = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
        f32 = (384.0 * torch.rand(B, 3, h, w, generator=g) - 64.0).float()      # both signs, beyond the byte range: the clamp is used
        return u8.numpy(), f32.numpy(), (win or (0, 0, h, w)), size
    B, (h, w), cons, with_mask = PREP_CASES[name]
    img = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    mask = (torch.rand(B, 1, h, w, generator=g) < 0.8).to(torch.uint8) if with_mask else None
    f = 0.9 * max(h, w) + 4.0 * torch.rand(B, 2, generator=g)
    c = torch.tensor([w / 2.0, h / 2.0]) + 3.0 * torch.rand(B, 2, generator=g) - 1.5
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f[:, 0], f[:, 1], c[:, 0], c[:, 1], 1.0
    return img.numpy(), None if mask is None else mask.numpy(), K.numpy(), dict(CONSTRAINTS[cons])


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _filter(x, filt, dtype):
    dt = np.dtype(dtype).type
    x = np.abs(x).astype(dtype)
    if filt == "bilinear":
        return np.where(x < dt(1), (dt(1) - x).astype(dtype), dt(0)).astype(dtype)
    a = dt(-0.5)
    p1 = (((((a + dt(2)) * x).astype(dtype) - (a + dt(3))).astype(dtype) * x).astype(dtype) * x).astype(dtype) + dt(1)
    p2 = ((((((x - dt(5)).astype(dtype) * x).astype(dtype) + dt(8)).astype(dtype) * x).astype(dtype) - dt(4)).astype(dtype) * a)
    return np.where(x < dt(1), p1.astype(dtype), np.where(x < dt(2), p2.astype(dtype), dt(0))).astype(dtype)


def axis_table(n_in, n_out, filt, dtype, first=0, count=None, defect=None, n_image=None):
    """(xmin int64 [count], xsize int64 [count], weights dtype [count, T]) of the virtual destination indices first .. first + count of
    an axis of n_in window samples and n_out destination samples; weights past xsize are 0.  defect: a planted restatement defect
    ("unnormalised", "plain_support", "image_extent" with n_image = the image's extent) for the tests of the tests."""
    dt = np.dtype(dtype).type
    count = n_out - first if count is None else count
    i = np.arange(first, first + count)
    if n_in == n_out and defect is None:
        return i.astype(np.int64), np.ones(count, dtype=np.int64), np.ones((count, 1), dtype=dtype)
    n_scale = n_image if defect == "image_extent" else n_in
    scale = dt(n_scale) / dt(n_out)
    big = scale if scale >= dt(1) else dt(1)
    if defect == "plain_support":
        big = dt(1)
    support = dt((dt(2) if filt == "bilinear" else dt(4)) * dt(0.5)) * big
    inv = dt(1) / scale if scale >= dt(1) else dt(1)
    if defect == "plain_support":
        inv = dt(1)
    center = (scale * (i.astype(dtype) + dt(0.5)).astype(dtype)).astype(dtype)
    lo = np.trunc(((center - support).astype(dtype) + dt(0.5)).astype(dtype)).astype(np.int64)
    lo = np.maximum(lo, 0)
    hi = np.trunc(((center + support).astype(dtype) + dt(0.5)).astype(dtype)).astype(np.int64)
    hi = np.minimum(hi, n_in)
    lo = np.clip(lo, 0, n_in - 1)
    n = np.clip(hi - lo, 1, n_in - lo)
    n = np.minimum(n, 33)
    T = int(n.max())
    j = np.arange(T)[None, :]
    arg = ((((j + lo[:, None]).astype(dtype) - center[:, None]).astype(dtype) + dt(0.5)).astype(dtype) * inv).astype(dtype)
    w = _filter(arg, filt, dtype)
    valid = j < n[:, None]
    w = np.where(valid, w, dt(0)).astype(dtype)
    total = w[:, 0].copy()
    for t in range(1, T):
        total = np.where(valid[:, t], (total + w[:, t]).astype(dtype), total)
    if defect != "unnormalised":
        with np.errstate(all="ignore"):                     # a planted defect can leave a pixel without weight
            w = np.where(valid, (w / total[:, None]).astype(dtype), dt(0)).astype(dtype)
    return lo, n, w


def _pass(v, table, axis, dtype):
    """one separable pass along `axis` (-1 or -2): first product, then the taps in order, every operation rounded in dtype"""
    lo, n, w = table
    v = np.moveaxis(v, axis, -1)
    T = w.shape[1]
    with np.errstate(all="ignore"):
        acc = (w[:, 0] * v[..., lo]).astype(dtype)
        for t in range(1, T):
            idx = np.minimum(lo + t, v.shape[-1] - 1)
            nxt = (acc + (w[:, t] * v[..., idx]).astype(dtype)).astype(dtype)
            acc = np.where(t < n, nxt, acc)
    return np.moveaxis(acc, -1, axis)


def window_of(src, window, dtype):
    """src [..., h, w] -> the window [..., height, width] in dtype, zeros outside the image (ContextCrop.crop / TF.pad)."""
    top, left, height, width = window
    h, w = src.shape[-2:]
    out = np.zeros(src.shape[:-2] + (height, width), dtype=dtype)
    y0, y1, x0, x1 = max(top, 0), min(top + height, h), max(left, 0), min(left + width, w)
    if y1 > y0 and x1 > x0:
        out[..., y0 - top:y1 - top, x0 - left:x1 - left] = src[..., y0:y1, x0:x1].astype(dtype)
    return out


def restate(src, window, size, filt="bicubic", dtype=np.float32, virtual=None, origin=(0, 0), defect=None):
    """The value of ud_resize_aa: src [B,C,h,w] uint8 or fp32, window (top, left, height, width) or None, size (Hn, Wn) ->
    [B,C,Hn,Wn] in dtype.  virtual = (Ho, Wo) and origin = (dtop, dleft) select a destination window of a larger resize."""
    src = np.asarray(src.cpu() if isinstance(src, torch.Tensor) else src)
    h, w = src.shape[-2:]
    window = tuple(window) if window is not None else (0, 0, h, w)
    Hn, Wn = size
    Ho, Wo = virtual or size
    v = window_of(src, window, dtype)
    d = defect if defect in ("unnormalised", "plain_support", "image_extent") else None
    tx = axis_table(window[3], Wo, filt, dtype, origin[1], Wn, d, w)
    ty = axis_table(window[2], Ho, filt, dtype, origin[0], Hn, d, h)
    return _pass(_pass(v, tx, -1, dtype), ty, -2, dtype)


def to_u8(v, defect=None):
    """round half to even, clamp, cast (defect "half_up": floor(v + 0.5))"""
    r = np.floor(v + v.dtype.type(0.5)) if defect == "half_up" else np.rint(v)
    return np.clip(np.nan_to_num(r, nan=0.0), 0, 255).astype(np.uint8)


def normalise(u8, mean=MEAN, std=STD):
    """((float)u8 / 255 - mean[c]) * inv_std[c] in fp32, inv_std = 1 / std rounded to fp32 (the values prepare_test_batch passes)."""
    f32 = np.float32
    m = np.asarray(mean, dtype=f32).reshape(-1, 1, 1)
    s = (f32(1) / np.asarray(std, dtype=f32)).astype(f32).reshape(-1, 1, 1)
    return (((u8.astype(f32) / f32(255)).astype(f32) - m).astype(f32) * s).astype(f32)


def nearest_index(n_in, n_out, first=0, count=None):
    """F.interpolate(mode="nearest") source indices: min((int)floorf((float)o * ((float)in / (float)out)), in - 1)"""
    f32 = np.float32
    count = n_out - first if count is None else count
    o = np.arange(first, first + count).astype(f32)
    return np.clip(np.floor((o * (f32(n_in) / f32(n_out))).astype(f32)).astype(np.int64), 0, n_in - 1)


def restate_mask(mask, hw, window, size, B=1, virtual=None, origin=(0, 0)):
    """the mask plane: mask uint8 [B,1,h,w] or None (all ones) -> uint8 [B,1,Hn,Wn]"""
    h, w = hw
    window = tuple(window) if window is not None else (0, 0, h, w)
    m = np.ones((B, 1, h, w), dtype=np.uint8) if mask is None else np.asarray(mask)
    win = window_of(m, window, np.uint8)
    Ho, Wo = virtual or size
    iy = nearest_index(window[2], Ho, origin[0], size[0])
    ix = nearest_index(window[3], Wo, origin[1], size[1])
    return win[..., iy, :][..., ix]


def restate_camera(K, window, Ho):
    """the intrinsics part: K fp32 [B,3,3] -> fp32 [B,3,3] (crop by (left, top), then the first two rows times zoom = Ho / height)"""
    f32 = np.float32
    K = np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K).astype(f32).reshape(-1, 3, 3).copy()
    top, left, height, _ = window
    zoom = f32(float(Ho) / float(height))
    K[:, 0, 2] = K[:, 0, 2] - f32(left)
    K[:, 1, 2] = K[:, 1, 2] - f32(top)
    K[:, :2, :] = (K[:, :2, :] * zoom).astype(f32)
    return K


def torch_composition(x, window, size, filt="bicubic", out="f32", mean=MEAN, std=STD):
    """What a user of the engine writes without ud_resize_aa, per plane: slice, F.pad, F.interpolate(antialias=True), and for the
    uint8 / normalised forms round, clamp, /255, normalise (torch tensors in and out, any device)."""
    import torch.nn.functional as F
    h, w = x.shape[-2:]
    top, left, height, width = window if window is not None else (0, 0, h, w)
    planes = []
    for b in range(x.shape[0]):
        per_c = []
        for c in range(x.shape[1]):
            p = x[b:b + 1, c:c + 1, max(top, 0):max(top + height, 0), max(left, 0):max(left + width, 0)].float()
            ph, pw = p.shape[-2:]
            pl = min(max(-left, 0), width)
            pt = min(max(-top, 0), height)
            p = F.pad(p, (pl, width - pl - pw, pt, height - pt - ph))
            p = F.interpolate(p, size=tuple(size), mode=filt, antialias=True, align_corners=False)
            if out != "f32":
                p = p.round().clamp(0, 255)
            if out == "u8":
                p = p.to(torch.uint8)
            if out == "norm":
                p = (p / 255 - mean[c]) / std[c]
            per_c.append(p)
        planes.append(torch.cat(per_c, dim=1))
    return torch.cat(planes)


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def _tv_shim():
    """torchvision.transforms.v2.functional as far as ContextCrop's test branch uses it (see the module docstring)."""
    import enum

    import torch.nn.functional as F

    class InterpolationMode(enum.Enum):
        NEAREST = "nearest"
        BILINEAR = "bilinear"
        BICUBIC = "bicubic"

    def resize(img, size, interpolation=InterpolationMode.BILINEAR, max_size=None, antialias=True):
        size = [int(v) for v in size]
        x = img.reshape((-1,) + tuple(img.shape[-3:]))
        if interpolation == InterpolationMode.NEAREST:
            out = F.interpolate(x.float(), size=size, mode="nearest").to(img.dtype)
        else:
            out = F.interpolate(x.float(), size=size, mode=interpolation.value, antialias=bool(antialias), align_corners=False)
            if img.dtype == torch.uint8:
                out = out.round().clamp(0, 255).to(torch.uint8)
            else:
                out = out.to(img.dtype)
        return out.reshape(tuple(img.shape[:-2]) + tuple(size))

    def pad(img, padding, fill=0, padding_mode="constant"):
        left, top, right, bottom = (int(v) for v in padding)
        return F.pad(img, (left, right, top, bottom), value=fill)

    m = types.ModuleType("torchvision.transforms.v2.functional")
    m.InterpolationMode, m.resize, m.pad = InterpolationMode, resize, pad
    return m


def reference_modules():
    """(transforms module, camera module) of the reference: transforms.py loaded by file path with the stand-in above as its TF."""
    import importlib
    import importlib.util
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    assert ref_loader.available(), "reference tree not present"
    ref_loader._prepare()
    shim = _tv_shim()
    stub = importlib.import_module("torchvision.transforms.v2.functional")       # the oracle's stub: keeps what other modules import
    for k, v in vars(stub).items():
        if not k.startswith("__") and not hasattr(shim, k):
            setattr(shim, k, v)
    sys.modules["torchvision.transforms.v2.functional"] = shim
    sys.modules["torchvision.transforms.v2"].functional = shim
    camera = importlib.import_module("unidepth.utils.camera")
    spec = importlib.util.spec_from_file_location("_ref_transforms", os.path.join(ref_loader.REF_ROOT, REF_TRANSFORMS))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, camera


def _rounded_image_shape(cons):
    m = cons["shape_mult"]
    return [-(-IMAGE_SHAPE[0] // m) * m, -(-IMAGE_SHAPE[1] // m) * m]           # base_dataset's rounding up to multiples of shape_mult


def reference_context_crop(mods, image, mask, K, cons):
    """The reference's ContextCrop(keep_original=True) on one sequence: image uint8 [B,3,h,w] -> dict of its outputs (numpy), plus the
    window it passed to crop()."""
    tr, cam = mods
    cc = tr.ContextCrop(image_shape=_rounded_image_shape(cons), keep_original=True, shape_constraints=dict(cons))
    seen = []
    real_crop = tr.ContextCrop.crop

    def crop(img, height, width, top, left):
        seen.append((int(top), int(left), int(height), int(width)))
        return real_crop(img, height=height, width=width, top=top, left=left)

    cc.crop = crop
    B = image.shape[0]
    Kt = torch.from_numpy(np.asarray(K)).clone()
    cams = [cam.BatchCamera.from_camera(cam.Pinhole(K=Kt[b:b + 1].clone())) for b in range(B)]
    results = dict(image=torch.from_numpy(np.asarray(image)).clone(), camera=torch.cat(cams) if B > 1 else cams[0],
                   image_fields={"image"}, mask_fields=set(), gt_fields=set(), camera_fields={"camera"})
    if mask is not None:
        results["validity_mask"] = torch.from_numpy(np.asarray(mask)).clone()
    out = cc(results)
    assert len(set(seen)) == 1
    return dict(image=out["image"].numpy(), mask=out["validity_mask"].numpy(), K=out["camera"].K.float().numpy(),
                shape=np.asarray(out["resized_shape"][0], dtype=np.int64), window=np.asarray(seen[0], dtype=np.int64),
                paddings=np.asarray(out["paddings"][0], dtype=np.int64), zoom=np.float64(out["image_rescale"]))


def main():
    mods = reference_modules()
    tr = mods[0]
    TF = sys.modules["torchvision.transforms.v2.functional"]
    out = {}
    for name in WINDOW_CASES:
        u8, f32, (top, left, height, width), size = case_inputs(name)
        for filt in FILTERS:
            mode = TF.InterpolationMode.BICUBIC if filt == "bicubic" else TF.InterpolationMode.BILINEAR
            cu = tr.ContextCrop.crop(torch.from_numpy(u8), height=height, width=width, top=top, left=left)
            cf = tr.ContextCrop.crop(torch.from_numpy(f32), height=height, width=width, top=top, left=left)
            out[f"{name}.{filt}.u8"] = TF.resize(cu, size, interpolation=mode, antialias=True).numpy()
            out[f"{name}.{filt}.u8_f32"] = TF.resize(cu.float(), size, interpolation=mode, antialias=True).numpy()
            out[f"{name}.{filt}.f32"] = TF.resize(cf, size, interpolation=mode, antialias=True).numpy()
    for cname in GEOMETRY_SETS:
        for (h, w) in GEOMETRY_SIZES:
            K = np.array([[[0.9 * max(h, w), 0, w / 2.0], [0, 0.9 * max(h, w), h / 2.0], [0, 0, 1]]], dtype=np.float32)
            r = reference_context_crop(mods, np.zeros((1, 3, h, w), dtype=np.uint8), None, K, CONSTRAINTS[cname])
            for k in ("shape", "window", "paddings", "zoom", "K"):
                out[f"geo.{cname}.{h}x{w}.{k}"] = r[k]
    for name in PREP_CASES:
        img, mask, K, cons = case_inputs(name)
        r = reference_context_crop(mods, img, mask, K, cons)
        for k, v in r.items():
            out[f"{name}.{k}"] = v
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
