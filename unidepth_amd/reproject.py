"""Point clouds back into images, over ud_splat / ud_splat_camera / ud_camera_project / ud_depth_minpool (include/unidepth_hip.h UdSplat,
UdSplatCamera, UdCameraProject, UdDepthMinPool; csrc/splat.hip, csrc/project.hip):

    render_depth, RenderedView      a batch of clouds (planar point maps, [B,N,3] rows or a packed PointCloud) splatted into depth maps
                                    through pinhole intrinsics and an optional rigid transform: z-buffer (nearest) or mean depth
    reproject                       render_depth on an infer() dict's `points`
    render_depth_camera             render_depth through any of the six camera models (one per image) instead of a pinhole matrix
    project_camera                  Camera.project for a batch: image coordinates, the in-image test and the model's depth, one launch
    project_points, downsample      unidepth/utils/geometric.py:161-204, 208-224 (same names, arguments and result shapes)

Three launches for the whole batch (fill, splat, resolve), integer atomics only: bitwise reproducible, stream-ordered, and without any
host synchronisation.  Tensors must live on the GPU: there is no CPU path."""
from __future__ import annotations

import math
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _args, _lib
from .gtpoints import prepare_camera
from .ops import check, cur_stream, mk
from .pointcloud import PointCloud


@dataclass
class RenderedView:
    """depth fp32 [B,1,H,W] (0 where no point landed); rgb u8 or fp32 [B,3,H,W] (holes 0), index int32 [B,H,W] (the winning point's
    index inside its image, -1 for holes) and count int32 [B,H,W] (points kept per pixel): None unless asked for."""
    depth: torch.Tensor
    rgb: Optional[torch.Tensor] = None
    index: Optional[torch.Tensor] = None
    count: Optional[torch.Tensor] = None


def _render(fn, points, image_shape, projector, transform, image, mode, pixel_offset, rounding, depth_range, return_index, return_count,
            workspace, flags=0) -> RenderedView:
    """What render_depth and render_depth_camera share: the parsing of every argument but the projector's, the workspace, the outputs and
    the call.  projector(B, device) -> (descriptor class, entry point's name, {tensors of the projector}, {its other fields},
    the PreparedCamera whose model tags the descriptor takes, or None)."""
    H, W = _args.image_shape(fn, image_shape)
    offsets = None
    if isinstance(points, PointCloud):
        xyz, offsets = points.xyz, points.offsets
        if image is None and mode == "nearest":
            image = points.rgb
        if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"{fn}: PointCloud.xyz must be fp32 [rows,3]")
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.ndim != 1 or offsets.numel() < 2:
            raise ValueError(f"{fn}: PointCloud.offsets must be int64 [B+1]")
        B, n = offsets.numel() - 1, xyz.shape[0]
        strides, cshape = (0, 3, 1), (n, 3)
        xyz, offsets = xyz.contiguous(), offsets.contiguous()
    else:
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
            raise ValueError(f"{fn}: points must be an fp32 tensor or a PointCloud")
        B, n, _, _, strides = _args.layout(fn, "points", points, 3)
        if B <= 0:
            raise ValueError(f"{fn}: empty batch")
        xyz, cshape = points.contiguous(), tuple(points.shape)
    if mode not in ("nearest", "mean"):
        raise ValueError(f"{fn}: mode must be 'nearest' or 'mean', got {mode!r}")
    if rounding not in ("floor", "trunc"):
        raise ValueError(f"{fn}: rounding must be 'floor' or 'trunc', got {rounding!r}")
    desc_cls, entry, proj_tensors, proj_fields, cam = projector(B, xyz.device)
    tensors = {"xyz": xyz, **proj_tensors}
    if offsets is not None:
        tensors["offsets"] = offsets
    T, nT = _args.rigid(fn, transform, B)
    if T is not None:
        tensors["T"] = T
    if image is not None:
        if mode == "mean":
            raise ValueError(f"{fn}: image needs mode='nearest' (a mean has no winning point to take a colour from)")
        if not isinstance(image, torch.Tensor) or image.dtype not in (torch.uint8, torch.float32) or tuple(image.shape) != cshape:
            raise ValueError(f"{fn}: image must be uint8 or fp32 {list(cshape)}, shaped like the points")
        tensors["color"] = image.contiguous()
    if return_index and mode == "mean":
        raise ValueError(f"{fn}: return_index needs mode='nearest'")
    flags |= _lib.UD_SPLAT_TRUNC if rounding == "trunc" else 0
    dmin = dmax = 0.0
    if depth_range is not None:
        try:
            dmin, dmax = (float(v) for v in depth_range)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: depth_range must be a (min, max) pair") from None
        flags |= _lib.UD_SPLAT_RANGE
    dev = xyz.device
    for name, t in tensors.items():
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{fn}: {name} must live on the GPU of the points ({dev}); there is no CPU path")
    if n == 0:                                         # an empty cloud has no address: one unread row stands in for it
        tensors["xyz"] = xyz.new_zeros(1, 3)
        if "color" in tensors:
            tensors["color"] = tensors["color"].new_zeros(1, 3)
    nbytes = int(_lib.lib.ud_splat_work_bytes(B, H, W))
    if nbytes < 0 or n > 2 ** 31 - 1:
        raise ValueError(f"{fn}: unsupported sizes B={B} H={H} W={W} points={n}")
    if workspace is None:
        workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous()
          or workspace.numel() < nbytes or workspace.data_ptr() % 8):
        raise ValueError(f"{fn}: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least {nbytes} bytes on {dev}")
    with torch.cuda.device(dev):
        depth = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
        rgb = torch.empty(B, 3, H, W, device=dev, dtype=image.dtype) if image is not None else None
        index = torch.empty(B, H, W, device=dev, dtype=torch.int32) if return_index else None
        count = torch.empty(B, H, W, device=dev, dtype=torch.int32) if return_count else None
        d = mk(desc_cls, depth=depth, rgb=rgb, index=index, count=count, work=workspace, work_bytes=workspace.numel(),
               batch_stride=strides[0], point_stride=strides[1], comp_stride=strides[2], n_points=n, B=B, H=H, W=W,
               nT=nT, mode=_lib.UD_SPLAT_MEAN if mode == "mean" else _lib.UD_SPLAT_NEAREST, flags=flags,
               color_f32=int(image is not None and image.dtype == torch.float32), pixel_offset=float(pixel_offset), dmin=dmin, dmax=dmax,
               **proj_fields, **tensors)
        if cam is not None:
            _args.set_models(d.model, cam)
        check(getattr(_lib.lib, entry)(d, cur_stream()), entry)
    return RenderedView(depth, rgb, index, count)


def render_depth(points, intrinsics: torch.Tensor, image_shape: Tuple[int, int], *, transform: Optional[torch.Tensor] = None,
                 image: Optional[torch.Tensor] = None, mode: str = "nearest", pixel_offset: float = 0.0, rounding: str = "floor",
                 depth_range=None, return_index: bool = False, return_count: bool = False,
                 workspace: Optional[torch.Tensor] = None) -> RenderedView:
    """Splat a batch of point clouds into (H, W) = image_shape depth maps.

    points: fp32 [B,3,h,w] (infer()'s planar point map), fp32 [B,N,3] (the reference's rows), or a PointCloud (packed rows of a batch;
    its device offsets say which image a row belongs to and are never read on the host).  intrinsics fp32 [3,3], [1,3,3] or [B,3,3]: the
    full matrix is applied, (a, b, w) = K (x, y, z), u = a / w + pixel_offset, v = b / w + pixel_offset.  transform fp32 [3,4] / [4,4]
    (or [1,..] / [B,..]): a rigid motion applied to the points first (source camera -> destination camera).  All in fp32, every
    operation rounded separately.

    pixel_offset: the continuous coordinate u covers pixel floor(u).  Use 0.5 for clouds unprojected at INTEGER pixel centres
    (pack_points in depth mode, get_pointcloud_from_rgbd: x = (u - cx) d / fx with u = 0, 1, ...): their points project back to integer
    coordinates give or take rounding, and the half pixel puts them in the middle of their own cell.  Use 0 for the reference's
    project_points convention, and for clouds whose pixel centres already sit at half-integer coordinates (infer()'s rays).
    rounding: "floor" (default), or "trunc" for the reference's .int(), which also takes u in (-1, 0) into column 0.

    mode "nearest": a z-buffer; points with z <= 0 are dropped, the smallest z wins a pixel and, among equal z, the smallest point
    index.  image (uint8 or fp32, shaped like the points: [B,3,h,w], [B,N,3], or [rows,3] for a PointCloud, where it defaults to the
    cloud's rgb) gives `rgb`, the winners' colours; return_index their indices.  mode "mean": the reference's mean depth per pixel
    (negative z allowed; an order-free fixed-point sum, exact to 2^-25 + one fp32 rounding); image and return_index are refused.
    depth_range (min, max) keeps min <= z <= max.  return_count: the number of kept points per pixel.
    workspace: an optional uint8 GPU tensor of at least ud_splat_work_bytes(B, H, W) bytes to reuse."""
    fn = "render_depth"

    def projector(B, dev):
        K = _args.matrices(fn, "intrinsics", intrinsics, B, 3, 3)
        return _lib.UdSplat, "ud_splat", {"K": K}, {"nK": K.shape[0]}, None
    return _render(fn, points, image_shape, projector, transform, image, mode, pixel_offset, rounding, depth_range, return_index,
                   return_count, workspace)


def _camera_rows(fn, camera, B, dev):
    """prepare_camera for the projecting functions: a CPU batch is refused here, in this module's words."""
    if dev.type != "cuda":
        raise ValueError(f"{fn}: points must live on the GPU; there is no CPU path")
    cam = prepare_camera(camera, B, dev)
    if cam.params.device != dev:
        raise ValueError(f"{fn}: the prepared camera lives on {cam.params.device}, the points on {dev}")
    return cam


def render_depth_camera(points, camera, image_shape: Tuple[int, int], *, transform: Optional[torch.Tensor] = None,
                        image: Optional[torch.Tensor] = None, mode: str = "nearest", pixel_offset: float = 0.0, rounding: str = "floor",
                        depth_range=None, max_angle: Optional[float] = None, return_index: bool = False, return_count: bool = False,
                        workspace: Optional[torch.Tensor] = None) -> RenderedView:
    """render_depth through a camera MODEL instead of a pinhole matrix (ud_splat_camera): every argument but `camera` and `max_angle` as
    in render_depth, the same three launches.  camera: anything gtpoints.prepare_camera takes -- an intrinsics tensor, a Pinhole / EUCM /
    Spherical / OPENCV / Fisheye624 / MEI, a BatchCamera (every image through its own member), or a PreparedCamera (under graph capture
    and in loops: nothing is copied from the host then).

    A point lands on the pixel of (u, v) = Camera.project(point) + pixel_offset.  Its depth -- what the z-buffer compares, the mean
    averages, depth_range tests and `depth` holds -- is the model's depth, the quantity gt_points multiplies with: z, or the distance
    |xyz| for Spherical.  So render_depth_camera(gt_points(depth, cam), cam, (H, W)) returns `depth`.  Every model but Spherical drops
    points with z <= 0, MEI those behind its mirror's horizon (z + xi |xyz| <= 0).  max_angle (radians): keep only points within that
    angle of the optical axis (z >= cos(max_angle) |xyz|; the cosine is taken on the host).  The polynomial models (OPENCV, Fisheye624,
    MEI) fold points far outside their field of view back into the image: this is how to cull them."""
    fn = "render_depth_camera"
    flags, cos_limit = 0, 0.0
    if max_angle is not None:
        try:
            cos_limit = math.cos(float(max_angle))
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: max_angle must be a number (radians)") from None
        flags = _lib.UD_SPLAT_FOV

    def projector(B, dev):
        cam = _camera_rows(fn, camera, B, dev)
        return _lib.UdSplatCamera, "ud_splat_camera", {"params": cam.params}, {"cos_limit": cos_limit}, cam
    return _render(fn, points, image_shape, projector, transform, image, mode, pixel_offset, rounding, depth_range, return_index,
                   return_count, workspace, flags)


def project_camera(points: torch.Tensor, camera, image_shape: Optional[Tuple[int, int]] = None, transform: Optional[torch.Tensor] = None):
    """Camera.project for a batch in one launch (ud_camera_project): points fp32 [B,3,h,w] or [B,N,3] on the GPU, camera as
    render_depth_camera takes it, one model per image -> (uv, inside, depth):

        uv      fp32 [B,2,h,w] / [B,N,2]   image coordinates (pixel centres at half-integers, as gt_points places them)
        inside  bool [B,h,w] / [B,N]       the model's own in-image test against image_shape = (H, W), comparisons as in the reference:
                                           Pinhole 0 <= u < W and 0 <= v < H; the others not (u < 0 or u > W or v < 0 or v > H), EUCM also
                                           not z < 0.  A NaN coordinate therefore counts as inside for every model but Pinhole.
        depth   fp32 [B,h,w] / [B,N]       the model's depth of the point: z, or |xyz| for Spherical

    image_shape defaults to (h, w) of a planar input and is required for rows.  transform fp32 [3,4] / [4,4] (or [1,..] / [B,..]) is
    applied to the points first.  Nothing synchronises; camera objects are uploaded with one small copy (capture with a PreparedCamera)."""
    fn = "project_camera"
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
        raise ValueError(f"{fn}: points must be an fp32 tensor")
    B, n, tail, rows, strides = _args.layout(fn, "points", points, 3)
    if image_shape is None:
        if rows:
            raise ValueError(f"{fn}: image_shape is required for [B,N,3] points")
        image_shape = tail
    H, W = _args.image_shape(fn, image_shape)
    if B <= 0:
        raise ValueError(f"{fn}: empty batch")
    if n > 2 ** 31 - 1:
        raise ValueError(f"{fn}: unsupported sizes B={B} points={n}")
    dev = points.device
    cam = _camera_rows(fn, camera, B, dev)
    xyz = points.contiguous()
    T, nT = _args.rigid(fn, transform, B)
    if T is not None and T.device != dev:
        raise ValueError(f"{fn}: T must live on the GPU of the points ({dev}); there is no CPU path")
    with torch.cuda.device(dev):
        uv = torch.empty((B, n, 2) if rows else (B, 2) + tail, device=dev, dtype=torch.float32)
        inside = torch.empty((B,) + tail, device=dev, dtype=torch.uint8)
        depth = torch.empty((B,) + tail, device=dev, dtype=torch.float32)
        if n:
            d = mk(_lib.UdCameraProject, xyz=xyz, params=cam.params, T=T, uv=uv, inside=inside, depth=depth, batch_stride=strides[0],
                   point_stride=strides[1], comp_stride=strides[2], n_points=n, B=B, H=H, W=W, nT=nT, uv_rows=rows)
            _args.set_models(d.model, cam)
            check(_lib.lib.ud_camera_project(d, cur_stream()), "ud_camera_project")
    return uv, inside.view(torch.bool), depth


def reproject(out, intrinsics: torch.Tensor, transform: Optional[torch.Tensor] = None, image_shape: Optional[Tuple[int, int]] = None,
              image: Optional[torch.Tensor] = None, **kw) -> RenderedView:
    """render_depth on an infer() dict of UniDepthV1 / V2: its `points` [B,3,h,w] seen through `intrinsics` after `transform`, into
    image_shape (default: the prediction's own h x w).  image [B,3,h,w] colours the view.  Usable as
    InferPipeline.submit(..., post=lambda o: views.append(reproject(o, K2, T12))): it runs on the call's stream."""
    if "points" not in out:
        raise ValueError("reproject: the prediction has no 'points'")
    pts = out["points"]
    if image_shape is None:
        if not isinstance(pts, torch.Tensor) or pts.ndim != 4:
            raise ValueError("reproject: the prediction's points must be [B,3,h,w]")
        image_shape = (pts.shape[2], pts.shape[3])
    return render_depth(pts, intrinsics, image_shape, transform=transform, image=image, **kw)


def project_points(points_3d: torch.Tensor, intrinsic_matrix: torch.Tensor, image_shape: Tuple[int, int]) -> torch.Tensor:
    """The reference's helper (utils/geometric.py:161-204): points_3d fp32 [B,N,3] through intrinsic_matrix [B,3,3] (the full matrix),
    pixel = int(u), int(v) (truncation), no culling by depth -> the mean z of the points of every pixel, fp32 [B,1,H,W], 0 where none
    landed.  Where the reference adds floats in scatter order, the sum here is an order-free fixed point (2^-24 steps, |z| <= 2^20):
    the same mean to 2^-25 plus one fp32 rounding, and the same bits on every run."""
    if not isinstance(points_3d, torch.Tensor) or points_3d.ndim != 3 or points_3d.shape[-1] != 3:
        raise ValueError("project_points: points_3d must be [B,N,3]")
    return render_depth(points_3d, intrinsic_matrix, image_shape, mode="mean", rounding="trunc", pixel_offset=0.0).depth


def downsample(data: torch.Tensor, downsample_factor: int = 2) -> torch.Tensor:
    """The reference's hole-aware min-pool of sparse depth maps (utils/geometric.py:208-224): data fp32 [N,1,H,W] -> [N,1,H/f,W/f], the
    minimum of every f x f block with zeros counted as 1e5, written as 0 when it exceeds 1000.  One launch, exact."""
    if not isinstance(data, torch.Tensor) or data.dtype != torch.float32 or data.ndim != 4 or data.shape[1] != 1:
        raise ValueError("downsample: data must be fp32 [N,1,H,W]")
    f = downsample_factor
    N, _, H, W = data.shape
    if not isinstance(f, int) or not 1 <= f <= 64 or N < 1 or N > 65535 or H < 1 or W < 1 or H % f or W % f or H * W > 2 ** 31 - 1:
        raise ValueError(f"downsample: factor must be an int in [1, 64] dividing H and W, 1 <= N <= 65535 (N={N}, H={H}, W={W}, factor={f})")
    if not data.is_cuda:
        raise ValueError("downsample: data must live on the GPU; there is no CPU path")
    src = data.contiguous()
    with torch.cuda.device(src.device):
        dst = torch.empty(N, 1, H // f, W // f, device=src.device, dtype=torch.float32)
        check(_lib.lib.ud_depth_minpool(mk(_lib.UdDepthMinPool, src=src, dst=dst, N=N, H=H, W=W, factor=f), cur_stream()), "ud_depth_minpool")
    return dst


class _CallableModule(type(sys)):
    """`unidepth_amd.reproject` names this module AND its function reproject(): importing the module binds it over the package's lazy
    attribute of the same name, so the module itself answers a call as the function does."""

    def __call__(self, *args, **kw):
        return reproject(*args, **kw)


sys.modules[__name__].__class__ = _CallableModule
