"""Surface normals of a point map or of a depth map seen through a camera, and the normal-error metrics of a batch -- what a demo shows
beside the depth, what a PLY needs before meshing, and the second table of the NYUv2 / iBims / ScanNet-style depth benchmarks.

    normals_from_points(points, ...)       one ud_normals call on infer()["points"] or any point map (csrc/normals.hip)
    normals_camera(depth, camera, ...)     the same from a depth and any of the six camera models, fused: the point map never reaches memory
    eval_normals(gt, pred, mask)           mean / median / rmse angular error and the shares below thresholds, per image, no host sync

The normal of a pixel is defined operation by operation in fp32 (csrc/normals_point.h), so a numpy restatement reproduces every bit.
The HIP kernels are the only implementation: CPU tensors raise."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _args, _lib
from .gtpoints import prepare_camera
from .ops import check, cur_stream, mk
from .unproject import unproject_camera


def _rtol(fn, edge_rtol):
    """(has_rtol, rtol_bits): the descriptor carries the fp32's bit pattern"""
    return (0, 0) if edge_rtol is None else (1, _args.tolerance(fn, "edge_rtol", edge_rtol)[1])


def _sizes(fn, B, H, W):
    _args.max_images(fn, B)
    _args.max_elems(fn, f"H={H} W={W}", H * W)
    if H > 524280:                                                    # the launch grid's rows of tiles
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
            _args.set_models(desc.model, cam)
        check(_lib.lib.ud_normals(desc, cur_stream()), "ud_normals")
    res = (normals,)
    if return_mask:
        res += (valid.view(torch.bool),)
    if return_rgb:
        res += (rgb,)
    return _args.tail(res)


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
    B, H, W = _args.point_map(fn, "points", points)
    _sizes(fn, B, H, W)
    if mask is not None:
        _args.image_map(fn, "mask", mask, H, W, mask=True, B=B)
    if depth is not None:
        _args.image_map(fn, "depth", depth, H, W, mask=False, B=B, shared=False)
    _rtol(fn, edge_rtol)
    dev = points.device
    _args.one_gpu(fn, dev, mask, depth)
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
    fn = "normals_camera"
    B, H, W = _args.depth_map(fn, "depth", depth)
    _sizes(fn, B, H, W)
    if mask is not None:
        _args.image_map(fn, "mask", mask, H, W, mask=True, B=B)
    _rtol(fn, edge_rtol)
    dev = depth.device
    _args.one_gpu(fn, dev, mask, *_args.prepared_rows(camera))
    with torch.cuda.device(dev):
        cam = prepare_camera(camera, B, dev)
        d = depth.reshape(B, H, W).float().contiguous()
        if _args.n_iterative(cam):                                # not fused: the radial loop ends on a maximum over the image
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
        _args.point_map(fn, name, t)
    if gt.shape != pred.shape:
        raise ValueError(f"{fn}: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} differ in shape")
    B, _, H, W = gt.shape
    _sizes(fn, B, H, W)
    if mask is not None:
        _args.image_map(fn, "mask", mask, H, W, mask=True, B=B)
    try:
        thr = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: thresholds must be a sequence of numbers") from None
    if not 1 <= len(thr) <= _lib.UD_EVAL_NORMALS_MAX_T:
        raise ValueError(f"{fn}: 1 to {_lib.UD_EVAL_NORMALS_MAX_T} thresholds, got {len(thr)}")
    if not all(math.isfinite(t) and 0.0 < t <= 180.0 for t in thr):
        raise ValueError(f"{fn}: thresholds must be angles in (0, 180] degrees, got {thr}")
    dev = gt.device
    _args.one_gpu(fn, dev, pred, mask)
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
            desc.cos_bits[k] = _args.f32_bits(math.cos(math.radians(t)))
        check(_lib.lib.ud_eval_normals(desc, work.data_ptr(), nbytes, cur_stream()), "ud_eval_normals")
    res = {"mean": out[0], "median": out[1], "rmse": out[2]}
    for k, t in enumerate(thresholds):
        res[f"a_{t}"] = out[3 + k]
    res["count"] = count
    if return_error:
        res["error"] = err
    return res
