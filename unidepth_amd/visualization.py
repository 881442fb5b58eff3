"""Depth maps as colour images, over ud_colorize (include/unidepth_hip.h UdColorize, csrc/colorize.hip):

    colorize, image_grid           unidepth/utils/visualization.py:17-54 (same names, arguments and results)
    colorize_batch                 a batch of maps -> uint8 images on the GPU, one call
    demo_panel                     the artifact of scripts/demo.py (rgb | gt / pred | error, or rgb | pred) for a whole batch, one call
    save_png                       8-bit RGB PNG with the standard library only
    preload_colormap               a colormap's table on a device ahead of its first use

The colormap tables are unidepth_amd/colormaps.py (generated from matplotlib by tools/make_colormaps.py; matplotlib is never imported
here).  The device calls are stream-ordered, bitwise reproducible and make no host synchronisation (but for the first use of a colormap on a
device, which uploads its table: preload_colormap does that ahead of time); tensors must live on the GPU: there is no CPU path for
tensors.  Arrays are coloured on the host in numpy, as the reference does."""
from __future__ import annotations

import struct
import zlib
from typing import Optional

import numpy as np
import torch

from . import _lib
from .colormaps import get_table
from .ops import check, cur_stream

_LUTS = {}                     # (colormap name, device) -> uint8 [256, 3] tensor on that device


def _lut(name, dev):
    key = (name, str(dev))
    if key not in _LUTS:
        t = torch.from_numpy(np.array(get_table(name))).to(dev)
        if t.is_cuda:                                    # the FIRST use of a colormap on a device uploads its table and waits for the copy
            torch.cuda.current_stream(t.device).synchronize()   # once: later calls may come from any stream
        _LUTS[key] = t
    return _LUTS[key]


def preload_colormap(cmap: str = "magma_r", device=None) -> None:
    """Uploads a colormap's table to `device` (default: the current GPU) now.  The first use of a colormap on a device copies its 768
    bytes and waits for the copy; after this call colorize / colorize_batch / demo_panel with that colormap never synchronise, which a
    post= hook of InferPipeline wants.  Call it once per colormap and device from the thread that sets the pipeline up."""
    get_table(cmap)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"preload_colormap: device must be a GPU, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    _lut(cmap, dev)


# ---- host ------------------------------------------------------------------------------------------------------------------------------

def _colorize_host(value: np.ndarray, vmin, vmax, cmap) -> np.ndarray:
    """ud_colorize's per-pixel arithmetic (include/unidepth_hip.h UdColorize) on one host array, every operation in the array's own
    floating dtype T (float64 for an integer array): lo = T(vmin), den = T(double(vmax) - double(vmin)) when both limits are given,
    else the array's own minimum / maximum (NaN if any pixel is NaN) and den = hi - lo in T."""
    lut = get_table(cmap)
    if value.ndim >= 3:
        if value.shape[-1] != 1:                         # [..., C] with C channels is an image already: handed back untouched
            return value
        value = value.reshape(value.shape[:-1])
    T = value.dtype.type if value.dtype.kind == "f" else np.float64
    v = value.astype(T, copy=False)
    with np.errstate(all="ignore"):
        if vmin is not None and vmax is not None:
            lo, den = T(vmin), T(float(vmax) - float(vmin))
        else:
            lo = T(v.min() if vmin is None else vmin)
            hi = T(v.max() if vmax is None else vmax)
            den = T(hi - lo)
        x = (v - lo) / den * T(256)
        black = np.isnan(x) | (v < T(1e-4))              # a NaN compares false: only x's NaN blackens it
        idx = np.where(x >= 256, 255, np.where(x > 0, x, 0)).astype(np.int64)    # NaN -> 0 here, blackened below; truncation of [0, 256)
    img = lut[idx]
    img[black] = 0
    return img


def colorize(value, vmin: Optional[float] = None, vmax: Optional[float] = None, cmap: str = "magma_r"):
    """The reference's colorize.  A numpy array [H,W] (or [H,W,1]; an array that is already RGB is returned as is) gives a uint8 [H,W,3]
    array computed on the host in the input's own dtype: float64 stays float64.  A GPU tensor fp32 [H,W], [B,H,W] or [B,1,H,W] goes
    through ud_colorize and gives a uint8 GPU tensor [H,W,3] / [B,H,W,3]; a limit left None is the image's own minimum / maximum, per
    image.  Pixels below 1e-4 are black; a NaN is black; a NaN under an automatic limit blackens its whole image."""
    if isinstance(value, torch.Tensor):
        if value.ndim not in (2, 3, 4) or (value.ndim == 4 and value.shape[1] != 1):
            raise ValueError(f"colorize: a tensor must be [H,W], [B,H,W] or [B,1,H,W], got {tuple(value.shape)}")
        out = colorize_batch(value[None] if value.ndim == 2 else value, vmin, vmax, cmap)
        return out[0] if value.ndim == 2 else out
    return _colorize_host(np.asarray(value), vmin, vmax, cmap)


def image_grid(imgs, rows: int, cols: int):
    """The reference's image_grid: rows x cols images, each the size of the first, pasted row-major into one uint8 [rows*h, cols*w, 3]
    array.  Equal sizes are pasted with numpy; differing sizes are resized bilinearly through PIL as in the reference, when PIL is
    importable.  An empty list gives None."""
    n = len(imgs)
    if n == 0:
        return None
    if n != rows * cols:
        raise ValueError(f"image_grid: {len(imgs)} images do not fill a {rows} x {cols} grid")
    imgs = [np.asarray(im) for im in imgs]
    h, w = imgs[0].shape[:2]
    if any(im.shape[:2] != (h, w) for im in imgs):
        try:
            from PIL import Image
        except ImportError:
            raise ValueError("image_grid: images of differing sizes need PIL for the resize, which is not importable") from None

        def fit(im):                                     # PIL's bilinear resize to the first image's size, as the reference's grid does
            pil = Image.fromarray(np.asarray(im, dtype=np.uint8))
            return np.asarray(pil.resize(size=(w, h), resample=Image.BILINEAR))

        imgs = [im if im.shape[:2] == (h, w) else fit(im) for im in imgs]
    grid = np.zeros((rows * h, cols * w, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        im = im.astype(np.uint8)
        if im.ndim == 2:
            im = im[..., None]
        if im.ndim != 3 or im.shape[2] not in (1, 3, 4):
            raise ValueError(f"image_grid: image {i} must be [h,w], [h,w,1], [h,w,3] or [h,w,4], got {im.shape}")
        r, c = divmod(i, cols)
        grid[r * h:(r + 1) * h, c * w:(c + 1) * w] = im[..., :3]
    return grid


def save_png(path, img) -> None:
    """8-bit RGB PNG of a uint8 [H,W,3] array or tensor (a [3,H,W] image is not guessed: pass HWC), written with zlib and struct only."""
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"save_png: img must be uint8 [H,W,3], got {img.dtype} {img.shape}")
    H, W = img.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)                  # filter type 0 in front of every scanline
    raw[:, 1:] = img.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


# ---- device ----------------------------------------------------------------------------------------------------------------------------

def _limit(fn, name, v):
    if v is None:
        return None
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {name} must be a number or None") from None


def _map_view(fn, name, t, B, H, W):
    """A fp32 map [B,H,W] / [B,1,H,W] whose images are dense -> (tensor to keep alive, batch stride in elements).  A batch-strided view
    (a channel of a larger tensor) is used in place; anything else is made contiguous."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{fn}: {name} must be a fp32 tensor")
    if tuple(t.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"{fn}: {name} must be [{B},1,{H},{W}] or [{B},{H},{W}], got {tuple(t.shape)}")
    t = t.reshape(B, H, W) if t.ndim == 3 else t[:, 0]
    dense = (W == 1 or t.stride(2) == 1) and (H == 1 or t.stride(1) == W)
    if not dense or (B > 1 and t.stride(0) < 0):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else 0)


def _panel_map(fn, t, stride, vmin, vmax, cmap, dev, second=None):
    p = _lib.UdColorPanel()
    p.kind = _lib.UD_CZ_MAP if second is None else _lib.UD_CZ_AREL
    p.src, p.batch_stride = t.data_ptr(), stride
    if second is not None:
        p.src2, p.batch_stride2 = second[0].data_ptr(), second[1]
    p.lut = _lut(cmap, dev).data_ptr()
    p.flags = (_lib.UD_CZ_AUTO_LO if vmin is None else 0) | (_lib.UD_CZ_AUTO_HI if vmax is None else 0)
    if vmin is not None:
        p.lo = vmin
    if vmax is not None:
        p.hi = vmax
    if vmin is not None and vmax is not None:
        p.den = vmax - vmin                                 # in double, then rounded to fp32 by the field: numpy's rule for Python floats
    return p


def _run(fn, panels, keep, B, H, W, rows, cols, dev, channels_first, out, workspace):
    shape = (B, 3, rows * H, cols * W) if channels_first else (B, rows * H, cols * W, 3)
    for name, t in keep.items():
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{fn}: {name} must live on the GPU of the first input ({dev}); there is no CPU path for tensors")
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f"{fn}: out must be a contiguous uint8 tensor {shape} on {dev}")
    d = _lib.UdColorize()
    auto = False
    for i, p in enumerate(panels):
        d.panels[i] = p
        auto = auto or bool(p.flags)
    if auto:
        nbytes = int(_lib.lib.ud_colorize_work_bytes(B, H, W))
        if nbytes < 0:
            raise ValueError(f"{fn}: unsupported sizes B={B} H={H} W={W}")
        if workspace is None:
            workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev
              or not workspace.is_contiguous() or workspace.numel() < nbytes):
            raise ValueError(f"{fn}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
        d.work, d.work_bytes = workspace.data_ptr(), workspace.numel()
    d.dst = out.data_ptr()
    d.B, d.H, d.W, d.rows, d.cols = B, H, W, rows, cols
    d.flags = _lib.UD_CZ_CHW if channels_first else 0
    with torch.cuda.device(dev):
        check(_lib.lib.ud_colorize(d, cur_stream()), "ud_colorize")
    return out


def colorize_batch(maps: torch.Tensor, vmin: Optional[float] = None, vmax: Optional[float] = None, cmap: str = "magma_r", *,
                   channels_first: bool = False, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """maps fp32 [B,H,W] or [B,1,H,W] on the GPU (a batch-strided view such as points[:, 2] is read in place) -> uint8 [B,H,W,3], or
    [B,3,H,W] with channels_first, in one ud_colorize call on the current stream.  A limit left None is each image's OWN minimum /
    maximum over all its pixels (what calling the reference once per image gives).  out: a uint8 tensor of the result's shape to write
    into.  workspace: an optional uint8 GPU tensor of at least ud_colorize_work_bytes(B, H, W) bytes (used by automatic limits)."""
    fn = "colorize_batch"
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.float32:
        raise ValueError(f"{fn}: maps must be a fp32 tensor")
    if maps.ndim not in (3, 4) or (maps.ndim == 4 and maps.shape[1] != 1):
        raise ValueError(f"{fn}: maps must be [B,H,W] or [B,1,H,W], got {tuple(maps.shape)}")
    B, H, W = maps.shape[0], maps.shape[-2], maps.shape[-1]
    if B <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"{fn}: empty input (B={B}, H={H}, W={W})")
    vmin, vmax = _limit(fn, "vmin", vmin), _limit(fn, "vmax", vmax)
    get_table(cmap)
    dev = maps.device
    t, stride = _map_view(fn, "maps", maps, B, H, W)
    return _run(fn, [_panel_map(fn, t, stride, vmin, vmax, cmap, dev)], {"maps": t}, B, H, W, 1, 1, dev, channels_first, out, workspace)


def demo_panel(rgb: torch.Tensor, depth_pred: torch.Tensor, depth_gt: Optional[torch.Tensor] = None, *, depth_range=(0.01, 10.0),
               error_range=(0.0, 0.2), cmap: str = "magma_r", error_cmap: str = "coolwarm", channels_first: bool = False) -> torch.Tensor:
    """The artifact of the reference's demo for a whole batch in one ud_colorize call: with depth_gt a 2 x 2 grid
    rgb | gt / pred | error (error = |gt - pred| / gt, 0 where gt == 0, coloured with error_cmap over error_range); without, 1 x 2
    rgb | pred.  rgb uint8 [B,3,H,W] (or [3,H,W]); depths fp32 [B,1,H,W] / [B,H,W] (or [H,W] with a single image).  A limit of a range
    may be None (per-image automatic).  Returns uint8 [B, rows*H, cols*W, 3], or [B, 3, rows*H, cols*W] with channels_first.  Usable as
    InferPipeline.submit(..., post=lambda o: panels.append(demo_panel(rgb, o["depth"]))): it runs on the call's stream."""
    fn = "demo_panel"
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.ndim not in (3, 4) or rgb.shape[-3] != 3:
        raise ValueError(f"{fn}: rgb must be a uint8 tensor [B,3,H,W] or [3,H,W]")
    if rgb.ndim == 3:
        rgb = rgb[None]
    B, _, H, W = rgb.shape
    if B <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"{fn}: empty input (B={B}, H={H}, W={W})")
    try:
        dlo, dhi = depth_range
        elo, ehi = error_range
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: depth_range and error_range must be (min, max) pairs") from None
    dlo, dhi, elo, ehi = (_limit(fn, n, v) for n, v in (("depth_range", dlo), ("depth_range", dhi), ("error_range", elo), ("error_range", ehi)))
    get_table(cmap)
    get_table(error_cmap)
    dev = rgb.device

    def dmap(name, t):
        if isinstance(t, torch.Tensor) and t.ndim == 2 and B == 1:
            t = t[None]
        return _map_view(fn, name, t, B, H, W)

    rgb = rgb.contiguous()
    pred, ps = dmap("depth_pred", depth_pred)
    keep = {"rgb": rgb, "depth_pred": pred}
    p_rgb = _lib.UdColorPanel()
    p_rgb.kind, p_rgb.src, p_rgb.batch_stride = _lib.UD_CZ_RGB, rgb.data_ptr(), 3 * H * W
    p_pred = _panel_map(fn, pred, ps, dlo, dhi, cmap, dev)
    if depth_gt is None:
        return _run(fn, [p_rgb, p_pred], keep, B, H, W, 1, 2, dev, channels_first, None, None)
    gt, gs = dmap("depth_gt", depth_gt)
    keep["depth_gt"] = gt
    panels = [p_rgb, _panel_map(fn, gt, gs, dlo, dhi, cmap, dev), p_pred, _panel_map(fn, gt, gs, elo, ehi, error_cmap, dev, second=(pred, ps))]
    return _run(fn, panels, keep, B, H, W, 2, 2, dev, channels_first, None, None)
