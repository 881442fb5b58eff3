"""Surface normals of a point map or of a depth map seen through a camera, and the normal-error metrics of a batch -- what a demo shows
beside the depth, what a PLY needs before meshing, and the second table of the NYUv2 / iBims / ScanNet-style depth benchmarks.

    normals_from_points(points, ...)       one ud_normals call on infer()["points"] or any point map (csrc/normals.hip)
    normals_camera(depth, camera, ...)     the same from a depth and any of the six camera models, fused: the point map never reaches memory
    eval_normals(gt, pred, mask)           mean / median / rmse angular error and the shares below thresholds, per image, no host sync

The normal of a pixel is defined operation by operation in fp32 (csrc/normals_point.h), so a numpy restatement reproduces every bit.
The HIP kernels are the only implementation: CPU tensors raise."""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence

import torch

from . import _lib
from .cameras import GT_FISHEYE624, GT_OPENCV
from .ops import check, cur_stream, mk

_GPU = "GPU tensors on one device expected (the HIP kernels are the only implementation)"
_ITERATIVE = (GT_OPENCV, GT_FISHEYE624)


def _f32_bits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _rtol(fn, edge_rtol):
    """(has_rtol, rtol_bits): the descriptor carries the fp32's bit pattern"""
    if edge_rtol is None:
        return 0, 0
    try:
        r = float(edge_rtol)
        bits = _f32_bits(r)
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: edge_rtol must be a number in fp32's range") from None
    if not (r >= 0.0 and math.isfinite(r)):
        raise ValueError(f"{fn}: edge_rtol must be finite and not negative, got {r}")
    return 1, bits


def _map(fn, name, t, B, H, W, float_ok, shared_ok):
    """a [B,1,H,W] / [B,H,W] map (a batch of 1 is shared where shared_ok): a mask (bool / uint8) or a depth (any float dtype) -> its batch"""
    kind = "a float" if float_ok else "a bool or uint8"
    good = isinstance(t, torch.Tensor) and (t.is_floating_point() if float_ok else t.dtype in (torch.bool, torch.uint8))
    if not good:
        raise ValueError(f"{fn}: {name} must be {kind} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.ndim not in (3, 4) or (t.ndim == 4 and t.shape[1] != 1) or tuple(t.shape[-2:]) != (H, W) or t.shape[0] not in ((1, B) if shared_ok else (B,)):
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} is not [B,1,{H},{W}] or [B,{H},{W}] with B = {B}{' or 1' if shared_ok else ''}")
    return t.shape[0]


def _sizes(fn, B, H, W):
    if B > _lib.UD_RECON_MAX_B:
        raise ValueError(f"{fn}: at most {_lib.UD_RECON_MAX_B} images per call, got {B}")
    if H * W >= 2 ** 31 - 4096 or H > 524280:
        raise ValueError(f"{fn}: unsupported sizes H={H} W={W}")


def _run(fn, *, points, depth, cam, mask, edge_rtol, return_mask, return_rgb, B, H, W, dev):
    has_rtol, rtol_bits = _rtol(fn, edge_rtol)
    with torch.cuda.device(dev):
        m = None if mask is None else mask.contiguous().view(torch.uint8)
        normals = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
        valid = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8) if return_mask else None
        rgb = torch.empty((B, 3, H, W), device=dev, dtype=torch.uint8) if return_rgb else None
        desc = mk(_lib.UdNormals, points=points, depth=depth, params=None if cam is None else cam.params, mask=m, normals=normals,
                  valid=valid, rgb=rgb, B=B, H=H, W=W, mask_shared=int(m is not None and m.shape[0] == 1 and B > 1), has_rtol=has_rtol,
                  rtol_bits=rtol_bits)
        if cam is not None:
            for b in range(B):
                desc.model[b] = cam.models[b]
        check(_lib.lib.ud_normals(desc, cur_stream()), "ud_normals")
    res = (normals,)
    if return_mask:
        res += (valid.view(torch.bool),)
    if return_rgb:
        res += (rgb,)
    return res if len(res) > 1 else res[0]


def normals_from_points(points: torch.Tensor, *, mask: Optional[torch.Tensor] = None, depth: Optional[torch.Tensor] = None,
                        edge_rtol: Optional[float] = None, return_mask: bool = False, return_rgb: bool = False):
    """The surface normal at every pixel of a point map, the whole batch in one launch.

    points     [B,3,H,W], any float dtype (converted to contiguous fp32): infer()'s `points`, gt_points' or any camera-frame point map.
    mask       bool / uint8 [B,1,H,W] or [B,H,W] (a batch of 1 is shared): pixels with 0 take no part.
    depth      [B,1,H,W] / [B,H,W], any float dtype: what the edge test compares; the points' z when absent (pack_points' choice).
    edge_rtol  a neighbour q of pixel c is dropped when not |d[c] - d[q]| <= edge_rtol * min(d[c], d[q]) (fp32; false for a NaN): no
               difference is taken across a depth step.

    A pixel is ok where the mask is set and its three coordinates are finite.  A neighbour (left, right, up, down) is usable when it is
    inside the image, ok and passes the edge test.  dx = P[right] - P[left], or the one-sided difference with the pixel itself when only
    one of the two is usable; dy the same with down and up.  n = cross(dy, dx), divided by its largest magnitude, then by its length,
    and negated when n . P > 0: every valid normal faces the viewer, also for mirrored or flip_y clouds (a fronto-parallel plane gives
    (0, 0, -1)).  A pixel is valid when it is ok, both differences exist and the cross product is non-zero and finite.  A 1 x W or
    H x 1 image has no valid pixel.  Every operation is one separately rounded fp32 operation (csrc/normals_point.h).

    ->  normals fp32 [B,3,H,W], exactly 0 where not valid; then, in this order,
        valid   bool [B,1,H,W] (return_mask=True)
        rgb     uint8 [B,3,H,W] (return_rgb=True): floor((n + 1) * 127.5 + 0.5) clamped to 0..255, 0 where not valid
        A tuple only when there is more than one.

    One launch, stream-ordered, nothing synchronises, no workspace: captures into a graph."""
    fn = "normals_from_points"
    if not isinstance(points, torch.Tensor) or not points.is_floating_point():
        raise ValueError(f"{fn}: points must be a float tensor, got {getattr(points, 'dtype', type(points).__name__)}")
    if points.ndim != 4 or points.shape[1] != 3 or min(points.shape) == 0:
        raise ValueError(f"{fn}: points must be [B,3,H,W], non-empty, got {tuple(points.shape)}")
    B, _, H, W = points.shape
    _sizes(fn, B, H, W)
    if mask is not None:
        _map(fn, "mask", mask, B, H, W, False, True)
    if depth is not None:
        _map(fn, "depth", depth, B, H, W, True, False)
    _rtol(fn, edge_rtol)
    dev = points.device
    if dev.type != "cuda" or any(t.device != dev for t in (mask, depth) if t is not None):
        raise RuntimeError(f"{fn}: {_GPU}")
    with torch.cuda.device(dev):
        p = points.float().contiguous()
        d = None if depth is None else depth.reshape(B, H, W).float().contiguous()
    return _run(fn, points=p, depth=d, cam=None, mask=mask, edge_rtol=edge_rtol, return_mask=return_mask, return_rgb=return_rgb,
                B=B, H=H, W=W, dev=dev)


def normals_camera(depth: torch.Tensor, camera, *, mask: Optional[torch.Tensor] = None, edge_rtol: Optional[float] = None,
                   return_mask: bool = False, return_rgb: bool = False):
    """The surface normals of a depth map seen through a camera: the bits of

        normals_from_points(gt_points(depth, camera), mask=mask & (depth > 0), depth=depth, edge_rtol=edge_rtol, ...)

    in ONE launch -- the points of a 32 x 8 tile and its one-pixel halo are reconstructed once into on-chip memory and the point map never
    reaches memory.

    depth    [B,1,H,W] or [B,H,W], any float dtype (converted to contiguous fp32); pixels with a depth that is not > 0 (NaN included)
             take no part.
    camera   as gtpoints.prepare_camera takes it: any of the six models, one per image; a PreparedCamera is accepted and nothing is copied
             from the host then (graph capture).
    mask, edge_rtol, return_mask, return_rgb and the outputs: normals_from_points'.  The edge test compares the depth itself (the
    distance for a Spherical camera, as gt_points takes it).

    One launch.  With an OPENCV or Fisheye624 member in the camera, whose radial loop ends on a maximum over the whole image, the points
    of the whole batch come from unproject_camera first and `depth > 0` is ANDed into the mask: five launches (three of
    unproject_camera, one comparison, the normals), six with a mask.  Stream-ordered, nothing synchronises: captures into a graph."""
    from .gtpoints import PreparedCamera, prepare_camera
    from .unproject import unproject_camera
    fn = "normals_camera"
    if not isinstance(depth, torch.Tensor) or not depth.is_floating_point():
        raise ValueError(f"{fn}: depth must be a float tensor, got {getattr(depth, 'dtype', type(depth).__name__)}")
    if depth.ndim not in (3, 4) or (depth.ndim == 4 and depth.shape[1] != 1) or min(depth.shape) == 0:
        raise ValueError(f"{fn}: depth must be [B,1,H,W] or [B,H,W], non-empty, got {tuple(depth.shape)}")
    B, (H, W) = depth.shape[0], depth.shape[-2:]
    _sizes(fn, B, H, W)
    if mask is not None:
        _map(fn, "mask", mask, B, H, W, False, True)
    _rtol(fn, edge_rtol)
    dev = depth.device
    others = [t for t in (mask,) if t is not None] + ([camera.params] if isinstance(camera, PreparedCamera) else [])
    if dev.type != "cuda" or any(t.device != dev for t in others):
        raise RuntimeError(f"{fn}: {_GPU}")
    with torch.cuda.device(dev):
        cam = prepare_camera(camera, B, dev)
        d = depth.reshape(B, H, W).float().contiguous()
        if any(m in _ITERATIVE for m in cam.models):              # not fused: the radial loop ends on a maximum over the image
            points = unproject_camera(None, cam, depth=d, image_shape=(H, W))
            positive = (d > 0).view(B, 1, H, W)
            mask = positive if mask is None else positive & mask.reshape(-1, 1, H, W).bool()
            return _run(fn, points=points.contiguous(), depth=d, cam=None, mask=mask, edge_rtol=edge_rtol, return_mask=return_mask,
                        return_rgb=return_rgb, B=B, H=H, W=W, dev=dev)
    return _run(fn, points=None, depth=d, cam=cam, mask=mask, edge_rtol=edge_rtol, return_mask=return_mask, return_rgb=return_rgb,
                B=B, H=H, W=W, dev=dev)


def eval_normals(gt: torch.Tensor, pred: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                 thresholds: Sequence[float] = (11.25, 22.5, 30.0), return_error: bool = False) -> dict:
    """The normal-error metrics of a batch, per image, without a host synchronisation.

    gt, pred     [B,3,H,W], any float dtype (converted to contiguous fp32); they need not be unit vectors.
    mask         bool / uint8 [B,1,H,W] or [B,H,W] (a batch of 1 is shared).
    thresholds   1 to 8 angles in degrees.

    A pixel counts where the mask is set, all six values are finite and both vectors have a length > 0 and finite.  Its cosine is
    c = ((gx*px + gy*py) + gz*pz) / (|g| * |p|) in fp32, clamped to [-1, 1]; its error acos(c).

    ->  dict of fp32 [B] tensors  mean, median, rmse (degrees; the median is the exact lower median, torch.median's)  and
        a_<threshold> for every threshold, keyed by str(threshold) ("a_11.25"): the share of pixels with an error strictly below it,
        counted as c > fp32(cos(threshold)); and  count  int64 [B].  An image without a usable pixel gets NaN and count 0.
        return_error=True adds  error  fp32 [B,1,H,W]: the error in degrees, NaN where the pixel does not count (colorize_batch shows it).

    Sums are fp64 in a fixed order and counts are integers: two calls give the same bits.  Nine launches whatever B is; the workspace
    comes from torch's allocator.  Stream-ordered: captures into a graph."""
    fn = "eval_normals"
    for name, t in (("gt", gt), ("pred", pred)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"{fn}: {name} must be a float tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if t.ndim != 4 or t.shape[1] != 3 or min(t.shape) == 0:
            raise ValueError(f"{fn}: {name} must be [B,3,H,W], non-empty, got {tuple(t.shape)}")
    if gt.shape != pred.shape:
        raise ValueError(f"{fn}: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} differ in shape")
    B, _, H, W = gt.shape
    _sizes(fn, B, H, W)
    if mask is not None:
        _map(fn, "mask", mask, B, H, W, False, True)
    try:
        thr = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: thresholds must be a sequence of numbers") from None
    if not 1 <= len(thr) <= _lib.UD_EVAL_NORMALS_MAX_T:
        raise ValueError(f"{fn}: 1 to {_lib.UD_EVAL_NORMALS_MAX_T} thresholds, got {len(thr)}")
    if not all(math.isfinite(t) and 0.0 < t <= 180.0 for t in thr):
        raise ValueError(f"{fn}: thresholds must be angles in (0, 180] degrees, got {thr}")
    dev = gt.device
    if dev.type != "cuda" or any(t.device != dev for t in (pred, mask) if t is not None):
        raise RuntimeError(f"{fn}: {_GPU}")
    T = len(thr)
    with torch.cuda.device(dev):
        g, p = gt.float().contiguous(), pred.float().contiguous()
        m = None if mask is None else mask.contiguous().view(torch.uint8)
        out = torch.empty((3 + T, B), device=dev, dtype=torch.float32)
        count = torch.empty((B,), device=dev, dtype=torch.int64)
        err = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32) if return_error else None
        nbytes = int(_lib.lib.ud_eval_normals_work_bytes(B, H, W, T))
        if nbytes < 0:
            raise ValueError(f"{fn}: unsupported sizes B={B} H={H} W={W} T={T}")
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        desc = mk(_lib.UdEvalNormals, gt=g, pred=p, mask=m, out=out, count=count, error=err, B=B, H=H, W=W, T=T,
                  mask_shared=int(m is not None and m.shape[0] == 1 and B > 1))
        for k, t in enumerate(thr):
            desc.cos_bits[k] = _f32_bits(math.cos(math.radians(t)))
        check(_lib.lib.ud_eval_normals(desc, work.data_ptr(), nbytes, cur_stream()), "ud_eval_normals")
    res = {"mean": out[0], "median": out[1], "rmse": out[2]}
    for k, t in enumerate(thresholds):
        res[f"a_{t}"] = out[3 + k]
    res["count"] = count
    if return_error:
        res["error"] = err
    return res
