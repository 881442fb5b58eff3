"""Validation inputs from raw uint8 images, over ud_resize_aa (include/unidepth_hip.h UdResizeAA, csrc/testprep.hip):

    test_geometry        the test branch of ContextCrop.__call__ (datasets/pipelines/transforms.py:1195-1321, keep_original=True) with
                         base_dataset's rounding of image_shape: network shape, window, paddings, zoom -- pure Python
    prepare_test_batch   ContextCrop(keep_original=True), /255 and TF.normalize (datasets/image_dataset.py:132-159) as ONE launch:
                         (inputs, image_metas) ready for model(inputs, image_metas), i.e. UniDepthV2.forward_test
    resize_aa            F.interpolate(x, size, mode, antialias=True, align_corners=False) for fp32 and uint8, with a source window
    original_image       utils/validation.py:15-49: image and depth back at the ground truth's size

The reference does this on the CPU in its dataloader, plane by plane (slice, TF.pad, TF.resize on uint8, NEAREST for the mask, camera
crop and resize, then two more passes for /255 and the normalisation).  Here everything is stream-ordered device work without a
host synchronisation.  GPU tensors only: the HIP kernel is the only implementation."""
from __future__ import annotations

import ctypes as C
from math import ceil
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import cur_stream

__all__ = ["TestGeometry", "test_geometry", "prepare_test_batch", "resize_aa", "original_image"]

_FILTERS = {"bicubic": _lib.UD_RESIZE_BICUBIC, "bilinear": _lib.UD_RESIZE_BILINEAR}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class TestGeometry(NamedTuple):
    shape: Tuple[int, int]                      # (Hn, Wn), multiples of shape_mult
    window: Tuple[int, int, int, int]           # (top, left, height, width) in source pixels; may reach outside the image
    paddings: Tuple[int, int, int, int]         # what the reference stores in the metas, see test_geometry
    zoom: float                                 # image_rescale = Hn / height

    __test__ = False                            # not a test class, whatever its name starts with


def test_geometry(hw: Sequence[int], image_shape: Sequence[int], shape_constraints: dict) -> TestGeometry:
    """The geometry ContextCrop(image_shape, keep_original=True, shape_constraints) gives an h x w image.
    image_shape is first rounded up to multiples of shape_mult (base_dataset.py:78-82).  With shape_constraints["sample"] (default True)
    the network shape is test_closest_shape's: the image's patch count clamped to [pixels_min, pixels_max] / shape_mult^2, its aspect
    ratio clamped to ratio_bounds, h = round(sqrt(pixels / ratio)), w = int(h * ratio); otherwise the rounded image_shape.  The window
    (_get_crop_shapes with ctx = 1) has the network shape's aspect ratio, never cuts the image and is centred ((h - height) // 2).
    paddings are the reference's four numbers in the reference's order: it documents them as (left, top, right, bottom), and
    forward_test reads them so, but position 1 holds the padding BELOW the image and position 3 the padding ABOVE it (transforms.py:
    1285-1290); for a centred window the two differ by at most one pixel.  Kept as the reference computes them."""
    if len(tuple(hw)) != 2 or min(int(v) for v in hw) < 1:
        raise ValueError(f"test_geometry: hw must be (h, w) >= 1, got {hw}")
    if len(tuple(image_shape)) != 2 or min(int(v) for v in image_shape) < 1:
        raise ValueError(f"test_geometry: image_shape must be (H, W) >= 1, got {image_shape}")
    for key in ("shape_mult", "ratio_bounds", "pixels_min", "pixels_max"):
        if key not in shape_constraints:
            raise ValueError(f"test_geometry: shape_constraints lacks '{key}'")
    h, w = int(hw[0]), int(hw[1])
    mult = int(shape_constraints["shape_mult"])
    if mult < 1:
        raise ValueError(f"test_geometry: shape_constraints['shape_mult'] must be >= 1, got {mult}")
    shape = [ceil(image_shape[0] / mult) * mult, ceil(image_shape[1] / mult) * mult]
    input_ratio = w / h
    if shape_constraints.get("sample", True):
        lo, hi = shape_constraints["pixels_min"] / (mult * mult), shape_constraints["pixels_max"] / (mult * mult)
        pixels = max(min(int(ceil(h / mult * w / mult)), hi), lo)
        ratio = min(max(input_ratio, shape_constraints["ratio_bounds"][0]), shape_constraints["ratio_bounds"][1])
        hn = round((pixels / ratio) ** 0.5)
        shape = [int(hn) * mult, int(hn * ratio) * mult]
    if min(shape) < 1:
        raise ValueError(f"test_geometry: shape_constraints give an empty network shape {shape} for a {h} x {w} image")
    output_ratio = shape[1] / shape[0]
    if output_ratio <= input_ratio:
        new_w = float(w)                        # ctx = 1: the longer side is kept, the other one padded
        new_h = new_w / output_ratio
    else:
        new_h = float(h)
        new_w = new_h * output_ratio
    height, width = int(ceil(new_h - 0.5)), int(ceil(new_w - 0.5))
    top, left = (h - height) // 2, (w - width) // 2
    right, bottom = left + width, top + height
    paddings = (max(-left + min(0, right), 0), max(bottom - max(h, top), 0), max(right - max(w, left), 0), max(-top + min(0, bottom), 0))
    return TestGeometry((shape[0], shape[1]), (top, left, height, width), paddings, shape[0] / height)


test_geometry.__test__ = False                  # a library function, not a test, wherever it is imported


def _window(window, h, w, who):
    if window is None:
        return 0, 0, h, w
    try:
        top, left, height, width = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: window must be (top, left, height, width), got {window!r}") from None
    if height < 1 or width < 1:
        raise ValueError(f"{who}: window {window} is empty")
    return top, left, height, width


def launch(src: torch.Tensor, dst: torch.Tensor, window, filt: int, out_form: int, *, virtual=None, origin=(0, 0), mask_src=None,
           mask_dst=None, K_in=None, K_out=None, mean=None, inv_std=None):
    """One ud_resize_aa on the current stream.  src [B,C,h,w] uint8 / fp32 contiguous; dst [B,C,Hn,Wn] fp32 or uint8 as out_form says, any
    view whose B * C * Hn * Wn elements are contiguous; window = (top, left, height, width); virtual = (Ho, Wo) and origin = (dtop, dleft)
    for a destination window.  The C-ABI validates the rest."""
    B, Cn, h, w = src.shape
    Hn, Wn = dst.shape[-2:]
    d = _lib.UdResizeAA()
    d.src, d.dst = src.data_ptr(), dst.data_ptr()
    d.mask_src = None if mask_src is None else mask_src.data_ptr()
    d.mask_dst = None if mask_dst is None else mask_dst.data_ptr()
    d.K_in = None if K_in is None else K_in.data_ptr()
    d.K_out = None if K_out is None else K_out.data_ptr()
    d.B, d.C, d.h, d.w = B, Cn, h, w
    d.top, d.left, d.height, d.width = window
    d.Ho, d.Wo = virtual or (Hn, Wn)
    d.dtop, d.dleft = origin
    d.Hn, d.Wn = Hn, Wn
    d.src_u8, d.filter, d.out_form = int(src.dtype == torch.uint8), filt, out_form
    for i in range(4):
        d.mean[i] = float(mean[i]) if mean is not None and i < len(mean) else 0.0
        d.inv_std[i] = float(inv_std[i]) if inv_std is not None and i < len(inv_std) else 1.0
    check(_lib.lib.ud_resize_aa(C.byref(d), cur_stream()), "ud_resize_aa")


def _check_scale(who, window, Ho, Wo):
    s = _lib.UD_RESIZE_MAX_SCALE
    if window[2] > s * Ho or window[3] > s * Wo:
        raise ValueError(f"{who}: size {Ho} x {Wo} shrinks the {window[2]} x {window[3]} window by more than {s} along an axis "
                         f"(the kernel's compile-time bound on the filter support)")


def resize_aa(x: torch.Tensor, size: Sequence[int], mode: str = "bicubic", window=None, out_dtype: Optional[torch.dtype] = None,
              *, virtual_size=None, origin=(0, 0)) -> torch.Tensor:
    """F.interpolate(x, size, mode=mode, antialias=True, align_corners=False) for x [B,C,h,w] fp32 or uint8, in one launch.
    window = (top, left, height, width): resize that window of x instead of all of it; it may reach outside x (zeros, as F.pad) or cut
    it.  out_dtype: torch.float32 or torch.uint8 (default: x's dtype); uint8 results are rounded half to even and clamped to [0, 255]
    -- torchvision's rule for a uint8 tensor.  virtual_size = (Ho, Wo) with origin = (top, left) returns the size-shaped window at
    `origin` of the resize to (Ho, Wo): a resize followed by a crop, without the pixels in between.  fp16 / bf16 inputs are
    computed in fp32 and cast back.  Down-scaling by more than 8 along an axis is refused (ValueError)."""
    if not isinstance(x, torch.Tensor) or x.ndim != 4 or min(x.shape) < 1:
        raise ValueError(f"resize_aa: x must be a non-empty [B,C,h,w] tensor, got {tuple(getattr(x, 'shape', ()))}")
    if mode not in _FILTERS:
        raise ValueError(f"resize_aa: mode {mode!r}: 'bicubic' or 'bilinear'")
    try:
        Hn, Wn = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"resize_aa: size must be (H, W), got {size!r}") from None
    if Hn < 1 or Wn < 1:
        raise ValueError(f"resize_aa: size {size} is empty")
    if x.dtype != torch.uint8 and not x.is_floating_point():
        raise ValueError(f"resize_aa: x must be uint8 or floating point, got {x.dtype}")
    out_dtype = out_dtype or x.dtype
    if out_dtype != torch.uint8 and not out_dtype.is_floating_point:
        raise ValueError(f"resize_aa: out_dtype must be uint8 or a floating point type, got {out_dtype}")
    B, Cn, h, w = x.shape
    win = _window(window, h, w, "resize_aa")
    Ho, Wo = (Hn, Wn) if virtual_size is None else (int(v) for v in virtual_size)
    dtop, dleft = (int(v) for v in origin)
    if dtop < 0 or dleft < 0 or dtop + Hn > Ho or dleft + Wn > Wo:
        raise ValueError(f"resize_aa: origin {origin} + size {size} does not fit virtual_size {(Ho, Wo)}")
    _check_scale("resize_aa", win, Ho, Wo)
    if not x.is_cuda:
        raise RuntimeError("resize_aa: GPU tensors expected (the HIP kernels are the only implementation)")
    with torch.cuda.device(x.device):
        src = x.detach()
        src = src.contiguous() if src.dtype == torch.uint8 else src.float().contiguous()
        u8 = out_dtype == torch.uint8
        out = torch.empty(B, Cn, Hn, Wn, dtype=torch.uint8 if u8 else torch.float32, device=x.device)
        launch(src, out, win, _FILTERS[mode], _lib.UD_RESIZE_OUT_U8 if u8 else _lib.UD_RESIZE_OUT_F32, virtual=(Ho, Wo), origin=(dtop, dleft))
    return out if u8 else out.to(out_dtype)


def _camera_matrix(camera, B, device):
    """camera of prepare_test_batch -> fp32 [B,3,3] on `device` (a copy), or None; device None: the argument checks alone"""
    from . import cameras
    if camera is None:
        return None
    if isinstance(camera, torch.Tensor):
        if camera.ndim not in (2, 3) or tuple(camera.shape[-2:]) != (3, 3):
            raise ValueError(f"prepare_test_batch: camera must be a [3,3] or [B,3,3] tensor or a Pinhole, got {tuple(camera.shape)}")
        K = camera.detach().reshape(-1, 3, 3)
    else:
        cam = cameras.as_camera(camera)
        if isinstance(cam, cameras.BatchCamera):
            uni = cam.uniform()
            if not isinstance(uni, cameras.Pinhole):
                other = next(type(c).__name__ for c in cam.cameras if not isinstance(c, cameras.Pinhole))
                raise NotImplementedError(f"prepare_test_batch: crop and resize of camera model '{other}' is not implemented (Pinhole is)")
            cam = uni
        if not isinstance(cam, cameras.Pinhole):
            raise NotImplementedError(f"prepare_test_batch: crop and resize of camera model '{type(cam).__name__}' is not implemented "
                                      f"(Pinhole is)")
        K = cam.K
    if K.shape[0] not in (1, B):
        raise ValueError(f"prepare_test_batch: camera holds {K.shape[0]} cameras for {B} images")
    if device is None:                              # validation only
        return K
    K = K.to(device=device, dtype=torch.float32, non_blocking=True)
    return K.expand(B, 3, 3).contiguous() if K.shape[0] != B else K.clone()


def prepare_test_batch(image: torch.Tensor, depth: Optional[torch.Tensor] = None, camera=None, validity_mask: Optional[torch.Tensor] = None,
                       *, image_shape: Sequence[int], shape_constraints: dict, mean: Sequence[float] = IMAGENET_MEAN,
                       std: Sequence[float] = IMAGENET_STD):
    """Raw uint8 images [B,3,h,w] -> (inputs, image_metas) for model(inputs, image_metas): what the reference's test dataloader
    yields as batch["data"], batch["img_metas"] (ContextCrop(keep_original=True), /255, TF.normalize), in ONE launch.
      inputs["image"]          fp32 [B,3,Hn,Wn]: the window of test_geometry resized (bicubic, antialiased), rounded to a byte as
                               torchvision does for uint8, / 255, normalised with mean / std
      inputs["validity_mask"]  uint8 [B,1,Hn,Wn]: validity_mask [B,1,h,w] (default: all ones) through the same window, NEAREST
      inputs["camera"]         fp32 [B,3,3], only with a camera ([3,3] / [B,3,3] tensor of the raw image, a cameras.Pinhole or a
                               reference Pinhole): cropped by the window and resized by zoom.  Like the reference, the camera is
                               left UNCHANGED when the image fills less than half of the window (its valid_area test, transforms.py:
                               1292-1312; with keep_original it does not retry).  The reference's second condition, a field of view
                               below 150 degrees after the crop, would need the intrinsics on the host and is not evaluated.
                               Other camera models raise NotImplementedError.
      inputs["depth"]          depth as given (forward_test uses its size only); absent when depth is None
      image_metas[i]           {"paddings": the reference's four numbers (see test_geometry), "image_rescale": zoom,
                               "resized_shape": (Hn, Wn), "image_ori_shape": (h, w)}
    No host synchronisation: the geometry is computed from shapes alone, so this can sit in front of InferPipeline.submit."""
    if not isinstance(image, torch.Tensor) or image.ndim != 4 or image.shape[1] != 3 or image.dtype != torch.uint8 or min(image.shape) < 1:
        raise ValueError(f"prepare_test_batch: image must be a uint8 [B,3,h,w] tensor, got {getattr(image, 'dtype', None)} "
                         f"{tuple(getattr(image, 'shape', ()))}")
    B, _, h, w = image.shape
    if validity_mask is not None and (not isinstance(validity_mask, torch.Tensor) or tuple(validity_mask.shape) != (B, 1, h, w)
                                      or validity_mask.dtype not in (torch.uint8, torch.bool)):
        raise ValueError(f"prepare_test_batch: validity_mask must be a uint8 or bool [{B},1,{h},{w}] tensor, got "
                         f"{getattr(validity_mask, 'dtype', None)} {tuple(getattr(validity_mask, 'shape', ()))}")
    if len(tuple(mean)) != 3 or len(tuple(std)) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError(f"prepare_test_batch: mean and std must be three numbers each, std non-zero, got {mean}, {std}")
    geo = test_geometry((h, w), image_shape, shape_constraints)
    (Hn, Wn), win = geo.shape, geo.window
    _check_scale("prepare_test_batch", win, Hn, Wn)
    _camera_matrix(camera, B, None)
    if not image.is_cuda:
        raise RuntimeError("prepare_test_batch: GPU tensors expected (the HIP kernels are the only implementation)")
    if validity_mask is not None and validity_mask.device != image.device:
        raise ValueError("prepare_test_batch: validity_mask must be on the image's device")
    dev = image.device
    f32 = torch.tensor(list(mean) + list(std), dtype=torch.float32)             # host arithmetic in fp32, as the kernel's definition states
    inv_std = (1.0 / f32[3:]).tolist()
    with torch.cuda.device(dev):
        K = _camera_matrix(camera, B, dev)
        pl, pb, pr, pt = geo.paddings
        follows = K is not None and h * w / (h + pb + pt) / (w + pl + pr) >= 0.5
        src = image.detach().contiguous()
        m = None if validity_mask is None else validity_mask.detach().contiguous().view(torch.uint8)
        out = torch.empty(B, 3, Hn, Wn, dtype=torch.float32, device=dev)
        mask = torch.empty(B, 1, Hn, Wn, dtype=torch.uint8, device=dev)
        launch(src, out, win, _lib.UD_RESIZE_BICUBIC, _lib.UD_RESIZE_OUT_NORM, mask_src=m, mask_dst=mask,
               K_in=K if follows else None, K_out=K if follows else None, mean=f32[:3].tolist(), inv_std=inv_std)
    inputs = {"image": out, "validity_mask": mask}
    if K is not None:
        inputs["camera"] = K
    if depth is not None:
        inputs["depth"] = depth
    metas = [{"paddings": list(geo.paddings), "image_rescale": geo.zoom, "resized_shape": [Hn, Wn], "image_ori_shape": (h, w)} for _ in range(B)]
    return inputs, metas


def _meta_paddings(metas, n):
    rows = []
    for m in metas:
        p = m.get("paddings", [0] * 4)
        p = p.tolist() if isinstance(p, torch.Tensor) else list(p)
        nested = p and isinstance(p[0], (list, tuple))
        for r in (p if nested else [p]):
            if len(r) != 4 or any(int(v) != v or v < 0 for v in r):
                raise ValueError(f"original_image: paddings must be four non-negative integers per image, got {r}")
            rows.append(tuple(int(v) for v in r))
    if not rows:
        rows = [(0, 0, 0, 0)]
    if len(set(rows)) != 1:
        raise ValueError(f"original_image: one padding for the whole batch expected (one window per call), got {sorted(set(rows))}")
    return rows[0]


def original_image(batch: dict, preds: Optional[dict] = None):
    """utils/validation.py:15-49: batch["data"]["image"] [B,3,Hn,Wn] and, if given, preds["depth"] resized (bilinear, antialiased,
    align_corners=False) to the ground truth's size plus the paddings of batch["img_metas"], then the paddings removed -- here one
    launch per map that computes only the pixels that remain (resize_aa with a destination window).  batch["data"]["depth"] [T,1,H,W]
    gives the size.  Returns (batch, preds), both updated in place like the reference.
    Paddings are read as (left, top, right, bottom).  The reference resizes to (H + top + bottom, W + right + top): its width takes the
    TOP padding where the left one belongs (line 28), and its `paddings[i]` indexes the stacked [B,4] tensor by image, not by side.
    Here the width is W + left + right, which is what the reference's expression gives whenever top == left -- zero paddings and
    paddings equal on all four sides in particular; for any other paddings this function returns the H x W result the reference's code
    aims at, where the reference itself returns a map of another width.  All images must share one padding."""
    if not isinstance(batch, dict) or "data" not in batch or "image" not in batch["data"] or "depth" not in batch["data"]:
        raise ValueError("original_image: batch must hold batch['data']['image'] and batch['data']['depth']")
    image, depth = batch["data"]["image"], batch["data"]["depth"]
    if not isinstance(depth, torch.Tensor) or depth.ndim != 4:
        raise ValueError(f"original_image: batch['data']['depth'] must be [T,1,H,W], got {tuple(getattr(depth, 'shape', ()))}")
    H, W = (int(v) for v in depth.shape[-2:])
    left, top, right, bottom = _meta_paddings(batch.get("img_metas", []), image.shape[0])
    kw = dict(mode="bilinear", virtual_size=(H + top + bottom, W + left + right), origin=(top, left))
    batch["data"]["image"] = resize_aa(image, (H, W), **kw)
    if preds is not None and "depth" in preds:
        preds["depth"] = resize_aa(preds["depth"], (H, W), **kw)
    return batch, preds
