"""The argument checks the camera-map wrappers share (gtpoints, unproject, reproject, remap, warp, normals, consistency, tsdf, icp): one sentence
per kind of fault, every message prefixed with the public name `fn` of the caller and naming the argument.  Nothing here touches the
device or launches anything; conversions stay in the wrappers."""
from __future__ import annotations

import math
import struct

import torch

from . import _lib
from .cameras import BatchCamera, GT_FISHEYE624, GT_OPENCV, as_camera

GPU = "GPU tensors on one device expected (the HIP kernels are the only implementation)"
ITERATIVE = (GT_OPENCV, GT_FISHEYE624)     # the models whose unprojection ends on a maximum over the whole image
MAX_ELEMS = 0x7FFFFFFF - 256               # UD_MAX_ELEMS of csrc/ud_common.h: element counts of one image stay below it


class PreparedCamera:
    """Parameter rows fp32 [B,16] on the device and the model tag of every image: what ud_reconstruct takes.  Made by
    gtpoints.prepare_camera(); gt_points accepts it in place of a camera and then copies nothing from the host."""

    def __init__(self, params: torch.Tensor, models):
        self.params, self.models = params, tuple(int(m) for m in models)

    def __len__(self):
        return len(self.models)


def n_cameras(camera) -> int:
    if isinstance(camera, PreparedCamera):
        return len(camera)
    if isinstance(camera, torch.Tensor):
        return camera.shape[0] if camera.ndim == 3 else 1
    cam = as_camera(camera)
    return len(cam.cameras) if isinstance(cam, BatchCamera) else cam.params.shape[0]


def camera_device(camera):
    t = camera if isinstance(camera, torch.Tensor) else getattr(camera, "params", None)
    return t.device if isinstance(t, torch.Tensor) else torch.device("cpu")


def prepared_rows(*cameras):
    """the device rows of the PreparedCamera arguments among `cameras`, for one_gpu (every other kind is uploaded by prepare_camera)"""
    return [c.params for c in cameras if isinstance(c, PreparedCamera)]


def _got(t):
    return getattr(t, "dtype", type(t).__name__)


def float_tensor(fn, name, t):
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise ValueError(f"{fn}: {name} must be a float tensor, got {_got(t)}")


def mask_tensor(fn, name, t):
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{fn}: {name} must be a bool or uint8 tensor, got {_got(t)}")


def batch_of(fn, name, k, B, shared=True):
    """one argument's batch k against the call's B; a batch of 1 is shared by every image where `shared`"""
    if k != B and not (shared and k == 1):
        raise ValueError(f"{fn}: {name} of {k} images for a batch of {B}" + (f" (1 or {B} expected)" if shared else ""))


def batches(fn, sizes: dict, B):
    for name, k in sizes.items():
        batch_of(fn, name, k, B)


def image_map(fn, name, t, H, W, *, mask, B=None, shared=True):
    """a [b,1,H,W] / [b,H,W] map of non-empty (H, W) images: a mask (bool / uint8) or, with mask=False, any float dtype -> b.
    With B the batch is checked here; without, the caller checks it once B is known."""
    (mask_tensor if mask else float_tensor)(fn, name, t)
    if t.ndim not in (3, 4) or t.shape[0] == 0 or tuple(t.shape[-2:]) != (H, W) or t.numel() != t.shape[0] * H * W:
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} is not [B,1,{H},{W}] or [B,{H},{W}]")
    if B is not None:
        batch_of(fn, name, t.shape[0], B, shared)
    return t.shape[0]


def per_point(fn, name, t, n, tail, rows):
    """image_map's rows-aware variant: a mask with one value per point, [b,1,H,W] / [b,H,W] for a planar uv, [b,N] for rows -> b"""
    mask_tensor(fn, name, t)
    if t.ndim < 2 or t.shape[0] == 0 or t.numel() != t.shape[0] * n or (rows and t.ndim != 2) or (not rows and tuple(t.shape[-2:]) != tail):
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} does not hold one value for each of the {tail} coordinates of every image")
    return t.shape[0]


def depth_map(fn, name, t):
    """a non-empty float [B,1,H,W] / [B,H,W] map that sets the call's sizes -> (B, H, W)"""
    float_tensor(fn, name, t)
    if t.ndim not in (3, 4) or (t.ndim == 4 and t.shape[1] != 1) or min(t.shape) == 0:
        raise ValueError(f"{fn}: {name} must be [B,1,H,W] or [B,H,W], non-empty, got {tuple(t.shape)}")
    return (t.shape[0],) + tuple(t.shape[-2:])


def point_map(fn, name, t):
    """a non-empty float [B,3,H,W] point map that sets the call's sizes -> (B, H, W)"""
    float_tensor(fn, name, t)
    if t.ndim != 4 or t.shape[1] != 3 or min(t.shape) == 0:
        raise ValueError(f"{fn}: {name} must be [B,3,H,W], non-empty, got {tuple(t.shape)}")
    return (t.shape[0],) + tuple(t.shape[-2:])


def layout(fn, name, t, C):
    """planar [B,C,H,W] or rows [B,N,C] -> (batch, points per image, (H, W) or (N,), rows flag, (batch, point, component) strides of
    the contiguous tensor).  C = 2: image coordinates; C = 3: points."""
    if t.ndim == 4 and t.shape[1] == C:
        tail, rows = tuple(t.shape[2:]), 0
        n = tail[0] * tail[1]
        return t.shape[0], n, tail, rows, (C * n, 1, n)
    if t.ndim == 3 and t.shape[2] == C:
        n = t.shape[1]
        return t.shape[0], n, (n,), 1, (C * n, C, 1)
    raise ValueError(f"{fn}: {name} must be [B,{C},H,W] or [B,N,{C}], got {tuple(t.shape)}")


def image_shape(fn, shape, name="image_shape"):
    try:
        H, W = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {name} must be (H, W)") from None
    if H <= 0 or W <= 0:
        raise ValueError(f"{fn}: {name} must be positive, got ({H}, {W})")
    return H, W


def matrices(fn, name, m, B, rows, cols):
    """fp32 [rows,cols], [1,rows,cols] or [B,rows,cols] -> contiguous [n,rows,cols]"""
    if not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or tuple(m.shape) not in ((rows, cols), (1, rows, cols), (B, rows, cols)):
        raise ValueError(f"{fn}: {name} must be fp32 [{rows},{cols}], [1,{rows},{cols}] or [{B},{rows},{cols}]")
    return m.reshape(-1, rows, cols).contiguous()


def rigid(fn, transform, B):
    """a rigid transform fp32 [3,4] / [4,4] (or [1,..] / [B,..]), or None -> (contiguous [nT,3,4], nT), or (None, 0)"""
    if transform is None:
        return None, 0
    if isinstance(transform, torch.Tensor) and transform.shape[-2:] == (4, 4):
        transform = transform[..., :3, :]
    T = matrices(fn, "transform", transform, B, 3, 4)
    return T, T.shape[0]


def f32_bits(v: float) -> int:
    """the bit pattern of v rounded to fp32, as the descriptors carry it"""
    return struct.unpack("<i", struct.pack("<f", v))[0]


def tolerance(fn, name, x):
    """a Python number as (the value of its fp32 rounding, that rounding's bit pattern); the rounded value is finite and >= 0"""
    try:
        bits = f32_bits(float(x))
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: {name} must be a number in fp32's range") from None
    val = struct.unpack("<f", struct.pack("<i", bits))[0]
    if not (val >= 0.0 and math.isfinite(val)):
        raise ValueError(f"{fn}: {name} must be finite and not negative, got {x}")
    return val, bits


def positive(fn, name, x) -> float:
    """a Python number that is finite and > 0 -> float"""
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {name} must be a number") from None
    if isinstance(x, bool) or not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{fn}: {name} must be finite and positive, got {x}")
    return v


def gate(fn, name, x) -> int:
    """a Python number as the bit pattern of its fp32 rounding; the rounded value is >= 0, +inf allowed, not a NaN"""
    try:
        v = float(x)
        bits = f32_bits(v) if math.isfinite(v) else f32_bits(math.copysign(math.inf, v)) if not math.isnan(v) else None
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: {name} must be a number in fp32's range or inf") from None
    if isinstance(x, bool) or bits is None or not v >= 0.0:
        raise ValueError(f"{fn}: {name} must not be negative or a NaN, got {x}")
    return bits


def radius(fn, r, most):
    if isinstance(r, bool) or not isinstance(r, int) or not 0 <= r <= most:
        raise ValueError(f"{fn}: radius must be an integer in 0 .. {most}, got {r!r}")


def levels(fn, L, H, W, most):
    """a pyramid of L levels over (H, W) images: every level keeps at least one pixel"""
    if isinstance(L, bool) or not isinstance(L, int) or not 1 <= L <= most:
        raise ValueError(f"{fn}: levels must be an integer in 1 .. {most}, got {L!r}")
    if min(H, W) < 2 ** (L - 1):
        raise ValueError(f"{fn}: {L} levels need H, W >= {2 ** (L - 1)}, got H={H} W={W}")


def max_images(fn, B):
    if B > _lib.UD_RECON_MAX_B:
        raise ValueError(f"{fn}: at most {_lib.UD_RECON_MAX_B} images per call, got {B}")


def max_elems(fn, what, *counts):
    """the element counts of one image against the limit of the entry points; `what` spells the sizes for the message"""
    if max(counts) >= MAX_ELEMS:
        raise ValueError(f"{fn}: unsupported sizes {what}")


def one_gpu(fn, dev, *others):
    """dev is a GPU and every other tensor (None entries skipped) lives on it"""
    if dev.type != "cuda" or any(t.device != dev for t in others if t is not None):
        raise RuntimeError(f"{fn}: {GPU}")


def n_iterative(*cams) -> int:
    """how many images of these PreparedCameras have an iterative model"""
    return sum(m in ITERATIVE for c in cams for m in c.models)


def set_models(array, cam, start=0):
    """the model tags of a PreparedCamera into a descriptor's model array"""
    for b, m in enumerate(cam.models):
        array[start + b] = m


def tail(res: tuple):
    """a tuple only when there is more than one result"""
    return res if len(res) > 1 else res[0]
