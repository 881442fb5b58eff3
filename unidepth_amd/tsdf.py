"""Depth views fused into a truncated signed distance (TSDF) volume and the volume's surface read back as points: the step after
depth_consistency when N predicted depth maps, their cameras and their poses become one scene (the result feeds save_ply).

    TsdfVolume                              tsdf, weight, optional colour, origin and voxel size of a batch of dense voxel grids
    tsdf_integrate(volume, depths, ...)     one ud_tsdf_integrate call (csrc/tsdf.hip): every voxel against every view, any camera model
    tsdf_integrate_composition(...)         the same definition spelled per view with project_camera, remap(mode="nearest") and torch
    tsdf_points(volume, ...)                the zero crossings between neighbouring voxels as a PointCloud (ud_tsdf_points)
    tsdf_render(volume, camera, size, ...)  the volume ray-cast from a camera: depth, valid, points, normals, colour (ud_tsdf_render,
                                            csrc/tsdf_render.hip); TsdfVolume.render forwards to it
    tsdf_render_composition(...)            the same definition spelled in torch, a loop over the samples of the march
    TsdfVolume.mesh(...)                    the surface as an indexed triangle mesh: tsdfmesh.tsdf_mesh (ud_tsdf_mesh, csrc/tsdf_mesh.hip)

For every voxel and every view, in view order: the voxel's centre moved into the view and projected, the view's depth read at the nearest
pixel, sdf = that depth - the centre's own depth, and where the pixel is valid and the voxel not further than `trunc` behind the surface,
min(sdf / trunc, 1) averaged into the voxel with the pixel's weight.  The fused kernel keeps the voxel's state in registers across all
views and every intermediate map out of memory; every output has the bits the composition gives.  The HIP kernels are the only
implementation of the fused form: CPU tensors raise.  Sequences longer than 256 image-view pairs are integrated by repeated calls on the
same volume (integrating views in one call or in several gives the same bits)."""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence

import torch

from . import _args, _lib
from .consistency import invert_rigid
from .gtpoints import PreparedCamera, prepare_camera
from .ops import check, cur_stream, mk
from .pointcloud import PointCloud, _packed
from .remap import remap
from .reproject import project_camera
from .unproject import unproject_camera

_FLT_MAX = 3.4028234663852886e38


class TsdfVolume:
    """A batch of B dense voxel grids of (Nz, Ny, Nx) voxels, x fastest: tsdf fp32 [B,Nz,Ny,Nx] (1 where nothing was seen), weight fp32
    [B,Nz,Ny,Nx] (0 there), color fp32 [B,3,Nz,Ny,Nx] or None, origin fp32 [1 or B,3] (the grid's corner in the volume's frame; the centre
    of voxel (ix, iy, iz) is origin + (index + 0.5) * voxel_size per axis) and voxel_size (a Python float, exactly representable in fp32)."""

    def __init__(self, tsdf: torch.Tensor, weight: torch.Tensor, color: Optional[torch.Tensor], origin: torch.Tensor, voxel_size: float):
        self.tsdf, self.weight, self.color, self.origin, self.voxel_size = tsdf, weight, color, origin, voxel_size

    def render(self, camera, size, transforms=None, **kw):
        """tsdf_render(self, camera, size, transforms, **kw)"""
        return tsdf_render(self, camera, size, transforms, **kw)

    def mesh(self, **kw):
        """tsdfmesh.tsdf_mesh(self, **kw): the surface as an indexed triangle mesh"""
        from .tsdfmesh import tsdf_mesh
        return tsdf_mesh(self, **kw)

    def track(self, depth, camera, size, transform, *, near, far, step=None, min_weight=1.0, **kw):
        """The pose of a new depth frame from the volume: the volume rendered at the prior pose -- self.render(camera, size, transform,
        near=near, far=far, return_points=True, return_normals=True) -- and icp.track_camera(depth, camera, points, normals, valid, camera,
        None, **kw) from the identity against that prediction (dist_tol is required; iters, cos_tol, normals, mask, weights, damping and
        min_count as there).

        transform   fp32 [4,4], [3,4] or [B,4,4] / [B,3,4]: the PRIOR pose, VOLUME (world) TO CAMERA coordinates, tsdf_integrate's and
                    tsdf_render's convention; for a video, the pose of the frame before.
        size        (H, W) of the rendered prediction; the depth frame may have another size when its camera says so.

        ->  (T_new fp32 [B,3,4], stats fp64 [B,iters,4]): the frame's pose, VOLUME (world) TO CAMERA coordinates again, so that
            tsdf_integrate(self, depth[:, None], [camera], T_new[:, None], ...) integrates the frame as it is.  track_camera's estimate
            E maps the frame camera to the prior camera, so T_new = invert_rigid(E) . transform, composed element-wise in fp32: row i of
            the product is ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j), plus a_i3 in the last column.  stats as track_camera returns them."""
        from .icp import track_camera
        fn = "TsdfVolume.track"
        B = _check_volume(fn, self)[0]
        _, valid, points, normals = self.render(camera, size, transform, near=near, far=far, step=step, min_weight=min_weight,
                                                return_points=True, return_normals=True)
        E, stats = track_camera(depth, camera, points, normals, valid, camera, None, **kw)
        return _tracked_pose(E, transform, B), stats

    def track_pyramid(self, depth, camera, size, transform, *, near, far, step=None, min_weight=1.0, levels=3, iters=(10, 5, 4), **kw):
        """track, coarse to fine: the volume rendered at the prior pose once per level, at (H >> l, W >> l) through
        pyramid.pyramid_cameras(camera, B, levels, device)[l], then pyramid.track_camera_pyramid(depth, those cameras, the renders, None,
        iters=iters, **kw) from the identity (dist_tol is required; filter, gate, cos_tol, mask, weights, damping and min_count as there).
        transform, size and the result: track's, composed the same way; stats fp64 [B,sum(iters),4] in execution order, coarsest level
        first.  A level whose iters entry is 0 is not rendered."""
        from .pyramid import pyramid_cameras, track_camera_pyramid
        fn = "TsdfVolume.track_pyramid"
        B = _check_volume(fn, self)[0]
        H, W = _args.image_shape(fn, size, "size")
        _args.levels(fn, levels, H, W, 4)
        cams = pyramid_cameras(camera, B, levels, self.tsdf.device)
        its = tuple(iters) if isinstance(iters, (tuple, list)) else iters
        model_levels = []
        for l in range(levels):
            if isinstance(its, tuple) and len(its) == levels and its[l] == 0:
                model_levels.append((None, None, None, cams[l]))
                continue
            _, valid, points, normals = self.render(cams[l], (H >> l, W >> l), transform, near=near, far=far, step=step, min_weight=min_weight,
                                                    return_points=True, return_normals=True)
            model_levels.append((points, normals, valid, cams[l]))
        E, stats = track_camera_pyramid(depth, cams, model_levels, None, iters=iters, **kw)
        return _tracked_pose(E, transform, B), stats


def _tracked_pose(E, transform, B):
    """track_camera's estimate E (frame camera -> prior camera) and the prior pose (volume -> camera) -> the frame's pose, volume -> camera:
    invert_rigid(E) . transform, composed element-wise in fp32 in the order TsdfVolume.track documents"""
    A = invert_rigid(E)
    if transform is None:
        return A
    Bm = transform[..., :3, :].reshape(-1, 3, 4)
    a = lambda i, j: A[:, i, j:j + 1]                            # noqa: E731
    rows = []
    for i in range(3):
        row = (a(i, 0) * Bm[:, 0] + a(i, 1) * Bm[:, 1]) + a(i, 2) * Bm[:, 2]
        rows.append(torch.cat([row[:, :3], row[:, 3:4] + a(i, 3)], dim=1))
    return torch.stack(rows, dim=1).expand(B, 3, 4).contiguous()


def _positive(fn, name, x):
    """a Python number as (the value of its fp32 rounding, that rounding's bit pattern); the rounded value is finite and > 0"""
    try:
        bits = _args.f32_bits(float(x))
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: {name} must be a number in fp32's range") from None
    val = struct.unpack("<f", struct.pack("<i", bits))[0]
    if isinstance(x, bool) or not (val > 0.0 and math.isfinite(val)):
        raise ValueError(f"{fn}: {name} must be finite and positive, got {x}")
    return val, bits


def _check_volume(fn, volume):
    """a TsdfVolume whose tensors are contiguous fp32 on one GPU and fit each other -> (B, Nz, Ny, Nx, voxel size, its bits)"""
    if not isinstance(volume, TsdfVolume):
        raise ValueError(f"{fn}: volume must be a TsdfVolume, got {type(volume).__name__}")
    t = volume.tsdf
    ok = lambda x: isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.device == t.device  # noqa: E731
    if not isinstance(t, torch.Tensor) or t.ndim != 4 or min(t.shape) == 0 or not ok(t):
        raise ValueError(f"{fn}: volume.tsdf must be a contiguous fp32 GPU tensor [B,Nz,Ny,Nx], non-empty")
    B, Nz, Ny, Nx = t.shape
    if not ok(volume.weight) or volume.weight.shape != t.shape:
        raise ValueError(f"{fn}: volume.weight must be a contiguous fp32 GPU tensor shaped like volume.tsdf {tuple(t.shape)}")
    if volume.color is not None and (not ok(volume.color) or tuple(volume.color.shape) != (B, 3, Nz, Ny, Nx)):
        raise ValueError(f"{fn}: volume.color must be None or a contiguous fp32 GPU tensor [{B},3,{Nz},{Ny},{Nx}]")
    if not ok(volume.origin) or tuple(volume.origin.shape) not in ((1, 3), (B, 3)):
        raise ValueError(f"{fn}: volume.origin must be a contiguous fp32 GPU tensor [1,3] or [{B},3]")
    vs, vs_bits = _positive(fn, "volume.voxel_size", volume.voxel_size)
    return B, Nz, Ny, Nx, vs, vs_bits


def _arguments(fn, volume, depths, cameras, transforms, grid_shape, origin, voxel_size, trunc, src_masks, src_weights, images, max_weight):
    """every check both functions share -> the sizes, the scalars and the tensors in the layout of the descriptor"""
    _args.float_tensor(fn, "depths", depths)
    if depths.ndim != 4 or min(depths.shape) == 0:
        raise ValueError(f"{fn}: depths must be [B,V,Hs,Ws], non-empty, got {tuple(depths.shape)}")
    B, V, Hs, Ws = depths.shape
    if V > 255 or B * V > _lib.UD_RECON_MAX_B:
        raise ValueError(f"{fn}: depths: at most 255 views and {_lib.UD_RECON_MAX_B} image-view pairs per call, got B={B} V={V}")
    if isinstance(cameras, (torch.Tensor, PreparedCamera)) or not isinstance(cameras, Sequence) or len(cameras) != V:
        raise ValueError(f"{fn}: cameras must be a sequence of {V} cameras, one per view")
    for v, cam in enumerate(cameras):
        _args.batch_of(fn, f"cameras[{v}]", _args.n_cameras(cam), B, shared=not isinstance(cam, PreparedCamera))
    shapes = ((V, 4, 4), (V, 3, 4), (B, V, 4, 4), (B, V, 3, 4))
    if not isinstance(transforms, torch.Tensor) or transforms.dtype != torch.float32 or tuple(transforms.shape) not in shapes:
        raise ValueError(f"{fn}: transforms must be fp32 [{V},4,4], [{B},{V},4,4] or the 3x4 forms of either")
    tr, tr_bits = _positive(fn, "trunc", trunc)
    has_max = max_weight is not None
    mw, mw_bits = _positive(fn, "max_weight", max_weight) if has_max else (0.0, 0)
    if src_masks is not None:
        _args.mask_tensor(fn, "src_masks", src_masks)
        if tuple(src_masks.shape) != (B, V, Hs, Ws):
            raise ValueError(f"{fn}: src_masks {tuple(src_masks.shape)} is not [{B},{V},{Hs},{Ws}]")
    if src_weights is not None:
        _args.float_tensor(fn, "src_weights", src_weights)
        if tuple(src_weights.shape) != (B, V, Hs, Ws):
            raise ValueError(f"{fn}: src_weights {tuple(src_weights.shape)} is not [{B},{V},{Hs},{Ws}]")
    if images is not None and (not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or tuple(images.shape) != (B, V, 3, Hs, Ws)):
        raise ValueError(f"{fn}: images must be uint8 [{B},{V},3,{Hs},{Ws}]")
    dev = depths.device
    fresh = volume is None
    if fresh:
        try:
            Nz, Ny, Nx = (int(k) for k in grid_shape)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: grid_shape must be (Nz, Ny, Nx) when no volume is given") from None
        if min(Nz, Ny, Nx) < 1:
            raise ValueError(f"{fn}: grid_shape must be positive, got ({Nz}, {Ny}, {Nx})")
        vs, vs_bits = _positive(fn, "voxel_size", voxel_size)
        if isinstance(origin, torch.Tensor):
            if origin.dtype != torch.float32 or tuple(origin.shape) not in ((3,), (1, 3), (B, 3)):
                raise ValueError(f"{fn}: origin must be fp32 [3], [1,3] or [{B},3], or three numbers")
        else:
            try:
                origin = torch.tensor([float(k) for k in origin], dtype=torch.float32)
            except (TypeError, ValueError):
                origin = None
            if origin is None or origin.shape != (3,):
                raise ValueError(f"{fn}: origin must be fp32 [3], [1,3] or [{B},3], or three numbers")
    else:
        if grid_shape is not None or origin is not None or voxel_size is not None:
            raise ValueError(f"{fn}: grid_shape, origin and voxel_size describe a fresh volume; a given volume carries its own")
        vb, Nz, Ny, Nx, vs, vs_bits = _check_volume(fn, volume)
        if vb != B:
            raise ValueError(f"{fn}: volume of {vb} grids for depths of {B} images")
        if (volume.color is None) != (images is None):
            raise ValueError(f"{fn}: images and volume.color go together (both or neither)")
    _args.max_elems(fn, f"grid={Nz}x{Ny}x{Nx} V={V} source={Hs}x{Ws}", Nx * Ny * Nz, V * 3 * Hs * Ws)
    _args.one_gpu(fn, dev, transforms, src_masks, src_weights, images, *(() if fresh else (volume.tsdf,)), *_args.prepared_rows(*cameras))
    with torch.cuda.device(dev):
        a = dict(B=B, V=V, Hs=Hs, Ws=Ws, Nz=Nz, Ny=Ny, Nx=Nx, vs=vs, vs_bits=vs_bits, trunc=tr, trunc_bits=tr_bits, has_max=has_max,
                 max_weight=mw, max_weight_bits=mw_bits, dev=dev, fresh=fresh, volume=volume)
        a["cams"] = [prepare_camera(c, B, dev) for c in cameras]
        a["src"] = depths.float().contiguous()
        a["T"] = transforms[..., :3, :].reshape(-1, V, 3, 4).contiguous()
        a["masks"] = None if src_masks is None else src_masks.contiguous().view(torch.uint8)
        a["weights"] = None if src_weights is None else src_weights.float().contiguous()
        a["images"] = None if images is None else images.contiguous()
        a["origin"] = origin.to(dev).reshape(-1, 3).contiguous() if fresh else volume.origin
    return a


def _result(a, tsdf, weight, color, count, return_count):
    volume = a["volume"] if not a["fresh"] else TsdfVolume(tsdf, weight, color, a["origin"], a["vs"])
    return (volume, count) if return_count else volume


def _centres(a):
    """the voxel centres fp32 [B,N,3], x fastest: origin + (index + 0.5) * voxel_size per axis"""
    dev, B = a["dev"], a["B"]
    shape = (a["Nz"], a["Ny"], a["Nx"])
    o = a["origin"]
    axes = []
    for k, (n, view) in enumerate(((a["Nx"], (1, 1, 1, -1)), (a["Ny"], (1, 1, -1, 1)), (a["Nz"], (1, -1, 1, 1)))):
        c = (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * a["vs"]
        axes.append((o[:, k].view(-1, 1, 1, 1) + c.view(view)).expand((o.shape[0],) + shape))
    return torch.stack(axes, dim=-1).reshape(o.shape[0], -1, 3).expand(B, -1, 3).contiguous()


def _compose(a, return_count):
    B, V, dev = a["B"], a["V"], a["dev"]
    shape = (B, a["Nz"], a["Ny"], a["Nx"])
    N = a["Nz"] * a["Ny"] * a["Nx"]
    with_color = a["images"] is not None
    if a["fresh"]:
        tsdf, W = torch.ones((B, N), device=dev), torch.zeros((B, N), device=dev)
        color = torch.zeros((B, 3, N), device=dev) if with_color else None
    else:
        vol = a["volume"]
        tsdf, W = vol.tsdf.reshape(B, N).clone(), vol.weight.reshape(B, N).clone()
        color = vol.color.reshape(B, 3, N).clone() if with_color else None
    count = torch.zeros((B, N), device=dev, dtype=torch.uint8)
    P = _centres(a)
    # divisors and bounds as device tensors: a division by a host scalar is a multiplication by its reciprocal
    trunc, one = torch.full((), a["trunc"], device=dev), torch.ones((), device=dev)
    max_w = torch.full((), a["max_weight"], device=dev)
    for v in range(V):
        sd = a["src"][:, v:v + 1]
        m = sd > 0
        if a["masks"] is not None:
            m = m & a["masks"][:, v:v + 1].bool()
        uv, inside, d = project_camera(P, a["cams"][v], (a["Hs"], a["Ws"]), transform=a["T"][:, v].contiguous())
        ds, valid = remap(sd, uv, mode="nearest", coord_valid=inside, src_mask=m, return_mask=True)
        ds = ds[..., 0]
        wv = one if a["weights"] is None else remap(a["weights"][:, v:v + 1], uv, mode="nearest", coord_valid=inside, src_mask=m)[..., 0]
        sdf = ds - d
        obs = valid & (d > 0) & (sdf >= -a["trunc"]) & (wv > 0) & (wv <= _FLT_MAX)
        s = torch.fmin(sdf / trunc, one)
        Wn = W + wv
        tsdf = torch.where(obs, (tsdf * W + s * wv) / Wn, tsdf)
        if with_color:
            rgb = remap(a["images"][:, v], uv, mode="nearest", coord_valid=inside, src_mask=m, out_dtype=torch.float32).permute(0, 2, 1)
            color = torch.where(obs[:, None], (color * W[:, None] + rgb * (wv if wv.ndim == 0 else wv[:, None])) / Wn[:, None], color)
        W = torch.where(obs, torch.fmin(Wn, max_w) if a["has_max"] else Wn, W)
        count = count + obs.to(torch.uint8)
    if not a["fresh"]:
        vol = a["volume"]
        vol.tsdf.copy_(tsdf.view(shape))
        vol.weight.copy_(W.view(shape))
        if with_color:
            vol.color.copy_(color.view(B, 3, *shape[1:]))
    return _result(a, tsdf.view(shape), W.view(shape), color.view(B, 3, *shape[1:]) if with_color else None, count.view(shape), return_count)


def tsdf_integrate_composition(volume: Optional[TsdfVolume], depths: torch.Tensor, cameras, transforms: torch.Tensor, *, grid_shape=None,
                               origin=None, voxel_size: Optional[float] = None, trunc: float, src_masks: Optional[torch.Tensor] = None,
                               src_weights: Optional[torch.Tensor] = None, images: Optional[torch.Tensor] = None,
                               max_weight: Optional[float] = None, return_count: bool = False):
    """tsdf_integrate's definition spelled with the separate calls, in a loop over the views: arguments and results as there.  The voxel
    centres are built in torch as [B,N,3] rows; per view project_camera(centres, cameras[v], (Hs, Ws), transform=transforms[v]) gives
    (u, v), inside and the centre's depth; remap(depths[:, v], uv, mode="nearest", coord_valid=inside, src_mask=(depths[:, v] > 0) &
    src_masks[:, v], return_mask=True) the sampled depth and its validity, and the same remap the weights and the colours; torch
    element-wise arithmetic, every operation a launch of its own, forms sdf, the decision and the running means.  Three library launches
    (up to five with weights and colours) and about twenty element-wise ones per view, each a pass over the whole volume.  This is the
    oracle of the fused kernel's tests and the counterpart of its benchmark."""
    a = _arguments("tsdf_integrate_composition", volume, depths, cameras, transforms, grid_shape, origin, voxel_size, trunc, src_masks,
                   src_weights, images, max_weight)
    with torch.cuda.device(a["dev"]):
        return _compose(a, return_count)


def tsdf_integrate(volume: Optional[TsdfVolume], depths: torch.Tensor, cameras, transforms: torch.Tensor, *, grid_shape=None, origin=None,
                   voxel_size: Optional[float] = None, trunc: float, src_masks: Optional[torch.Tensor] = None,
                   src_weights: Optional[torch.Tensor] = None, images: Optional[torch.Tensor] = None, max_weight: Optional[float] = None,
                   return_count: bool = False):
    """V depth views of each of B scenes averaged into B truncated signed distance volumes, the whole batch in one launch.

    volume       a TsdfVolume to update IN PLACE (its tensors contiguous fp32 on the GPU, else ValueError), or None: a fresh volume of
                 grid_shape = (Nz, Ny, Nx) voxels of voxel_size at origin (fp32 [3], [1,3] or [B,3], or three numbers: the grid's corner)
                 is made by the same single launch, without a memset.
    depths       [B,V,Hs,Ws] (any float dtype, converted to contiguous fp32), one size for all views.
    cameras      a sequence of V cameras, one per view, any of the six models.  Cameras are as gtpoints.prepare_camera takes them for B
                 images; a PreparedCamera is accepted and nothing is copied from the host then (graph capture).
    transforms   fp32 [V,4,4] or [B,V,4,4] (or the 3x4 forms): volume (world) to view-v-camera coordinates.
    trunc        the truncation distance, in the volume's units, rounded to fp32; a few voxel sizes.
    src_masks    bool / uint8 [B,V,Hs,Ws]: view pixels with 0 update nothing.
    src_weights  [B,V,Hs,Ws] (any float dtype): the weight of each pixel's observation, for example the network's confidence; 1 without.
                 A pixel whose weight is not a finite positive number updates nothing.
    images       uint8 [B,V,3,Hs,Ws]: the views' colours, averaged into volume.color with the same weights (a given volume must have
                 been made with images then, and only then).
    max_weight   the weight of a voxel is clamped to this after every update (a running mean that keeps adapting); None: no clamp.

    Voxel (ix, iy, iz) of volume b has the centre p = origin + (index + 0.5) * voxel_size per axis.  View v, in view order: q = T p,
    (u, w) its projection through the view's camera, d its depth (z, or the distance for Spherical); the view's depth ds at the nearest
    pixel (remap's mode="nearest"), valid as remap's `valid` for coord_valid = the camera's in-image test and src_mask = (depth > 0) &
    src_masks; sdf = ds - d.  The voxel is updated when valid, d > 0, sdf >= -trunc and the pixel's weight wv is finite and > 0 -- false
    whenever anything is a NaN: tsdf = (tsdf * W + min(sdf / trunc, 1) * wv) / (W + wv), the colour likewise, W = min(W + wv, max_weight).

    ->  the TsdfVolume (the given one, or the fresh one); with return_count=True (volume, count), count uint8 [B,Nz,Ny,Nx]: the views
        that updated each voxel in this call.

    One launch, plus the small one that stacks the views' parameter rows.  Stream-ordered, nothing synchronises, no workspace: captures
    into a graph (with PreparedCamera cameras).  At most 255 views and 256 image-view pairs per call: a longer sequence is integrated by
    repeated calls on the same volume, which gives the bits of one call over all views.  All six camera models are fused: there is no
    other path."""
    fn = "tsdf_integrate"
    a = _arguments(fn, volume, depths, cameras, transforms, grid_shape, origin, voxel_size, trunc, src_masks, src_weights, images, max_weight)
    B, V, dev = a["B"], a["V"], a["dev"]
    shape = (B, a["Nz"], a["Ny"], a["Nx"])
    with torch.cuda.device(dev):
        params = torch.stack([c.params for c in a["cams"]])                           # [V,B,16]
        if a["fresh"]:
            tsdf = torch.empty(shape, device=dev, dtype=torch.float32)
            weight = torch.empty(shape, device=dev, dtype=torch.float32)
            color = torch.empty((B, 3) + shape[1:], device=dev, dtype=torch.float32) if a["images"] is not None else None
        else:
            tsdf, weight, color = volume.tsdf, volume.weight, volume.color
        count = torch.empty(shape, device=dev, dtype=torch.uint8) if return_count else None
        desc = mk(_lib.UdTsdfIntegrate, src_depth=a["src"], src_mask=a["masks"], src_weight=a["weights"], image=a["images"], params=params,
                  T=a["T"], origin=a["origin"], tsdf=tsdf, weight=weight, color=color, count=count, B=B, V=V, Nx=a["Nx"], Ny=a["Ny"],
                  Nz=a["Nz"], Hs=a["Hs"], Ws=a["Ws"], nT=a["T"].shape[0], n_origin=a["origin"].shape[0], fresh=int(a["fresh"]),
                  has_max_weight=int(a["has_max"]), voxel_size_bits=a["vs_bits"], trunc_bits=a["trunc_bits"],
                  max_weight_bits=a["max_weight_bits"])
        for v in range(V):
            _args.set_models(desc.model, a["cams"][v], v * B)
        check(_lib.lib.ud_tsdf_integrate(desc, cur_stream()), "ud_tsdf_integrate")
    return _result(a, tsdf, weight, color, count, return_count)


def tsdf_points(volume: TsdfVolume, *, min_weight: float = 1.0, capacity: Optional[int] = None, rgb_dtype: torch.dtype = torch.uint8,
                workspace: Optional[torch.Tensor] = None) -> PointCloud:
    """The surface of a TsdfVolume as a packed PointCloud: one point per pair of neighbouring voxels (along +x, +y or +z) whose weights
    are both >= min_weight and whose distances a, b have different signs ((a < 0) != (b < 0), neither a NaN), at the linear zero crossing:
    the first voxel's centre moved by t * voxel_size along the axis, t = a / (a - b).  With volume.color the rows carry the colours
    c0 + t * (c1 - c0) as rgb_dtype: torch.uint8 (rounded half to even, clamped) or torch.float32.

    The order is fixed (volumes in batch order, then voxels x fastest, then the axes x, y, z) and every bit reproducible.
    capacity = int: outputs are [capacity, 3] and the call makes NO host synchronisation; counts / offsets still hold the true totals, so
    an overflow is detectable later.  capacity = None: counts first, reads the total back (one synchronisation) and allocates exactly
    that.  workspace: an optional uint8 GPU tensor of at least ud_tsdf_points_work_bytes(B, Nx, Ny, Nz) bytes to reuse.
    -> pointcloud.PointCloud (index is None); save_ply(path, cloud.xyz, cloud.rgb) takes it as it is."""
    fn = "tsdf_points"
    B, Nz, Ny, Nx, _, vs_bits = _check_volume(fn, volume)
    try:
        mw_bits = _args.f32_bits(float(min_weight))
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: min_weight must be a number in fp32's range") from None
    if isinstance(min_weight, bool) or math.isnan(float(min_weight)):
        raise ValueError(f"{fn}: min_weight must be a number, got {min_weight}")
    if rgb_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{fn}: rgb_dtype must be torch.uint8 or torch.float32, got {rgb_dtype}")
    nbytes = int(_lib.lib.ud_tsdf_points_work_bytes(B, Nx, Ny, Nz))
    if nbytes < 0:
        raise ValueError(f"{fn}: unsupported sizes B={B} grid={Nz}x{Ny}x{Nx} (3 * Nx * Ny * Nz must stay below 2^31 - 256)")

    def run(cap, xyz, rgb, index, **work):
        d = mk(_lib.UdTsdfPoints, tsdf=volume.tsdf, weight=volume.weight, color=volume.color, origin=volume.origin, xyz=xyz, rgb=rgb,
               capacity=cap, B=B, Nx=Nx, Ny=Ny, Nz=Nz, n_origin=volume.origin.shape[0], rgb_f32=int(rgb_dtype == torch.float32),
               voxel_size_bits=vs_bits, min_weight_bits=mw_bits, **work)
        check(_lib.lib.ud_tsdf_points(d, cur_stream()), "ud_tsdf_points")

    return _packed(fn, volume.tsdf.device, B, nbytes, run, capacity, workspace, None if volume.color is None else rgb_dtype, False)


# ---- the ray cast ------------------------------------------------------------------------------------------------------------------

_MAX_SAMPLES = 16384
# how ud_tsdf_render runs: a wave renders 64 pixels of a row (or an 8 x 8 pixel patch), and the samples that cannot lie in the grid are
# skipped (or all are visited).  No output bit depends on either; tools/bench_tsdf_render.py measures all four: rows with the clip is
# the fastest form at 256^3 (the patch takes 13 - 24 % longer), within 3.3 % of the fastest at 128^3 with B = 1, and up to 17 % slower
# than the unclipped patch at 128^3 with B = 8 (profiles/tsdf_render_bench.txt).
_RENDER_OPTIONS = dict(wave_patch=0, full_scan=0)


def _number(fn, name, x):
    """a Python number as (the value of its fp32 rounding, that rounding's bit pattern); not a NaN"""
    try:
        bits = _args.f32_bits(float(x))
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: {name} must be a number in fp32's range") from None
    val = struct.unpack("<f", struct.pack("<i", bits))[0]
    if isinstance(x, bool) or math.isnan(val):
        raise ValueError(f"{fn}: {name} must be a number, got {x}")
    return val, bits


def _render_arguments(fn, volume, camera, size, transforms, rays, near, far, step, min_weight, return_color, color_dtype):
    """every check both functions share -> the sizes, the scalars and the tensors in the layout of the descriptor"""
    B, Nz, Ny, Nx, vs, vs_bits = _check_volume(fn, volume)
    Ho, Wo = _args.image_shape(fn, size, "size")
    if camera is None:
        raise ValueError(f"{fn}: camera must be a camera for {B} images (with rays it still selects the depth: distance or z)")
    _args.batch_of(fn, "camera", _args.n_cameras(camera), B, shared=not isinstance(camera, PreparedCamera))
    T = None
    if transforms is not None:
        shapes = ((4, 4), (3, 4), (1, 4, 4), (1, 3, 4), (B, 4, 4), (B, 3, 4))
        if not isinstance(transforms, torch.Tensor) or transforms.dtype != torch.float32 or tuple(transforms.shape) not in shapes:
            raise ValueError(f"{fn}: transforms must be None or fp32 [4,4], [3,4], [{B},4,4] or [{B},3,4]")
        T = transforms[..., :3, :].reshape(-1, 3, 4)
    if rays is not None and (not isinstance(rays, torch.Tensor) or rays.dtype != torch.float32 or tuple(rays.shape) != (B, 3, Ho, Wo)):
        raise ValueError(f"{fn}: rays must be None or fp32 [{B},3,{Ho},{Wo}]")
    nr, nr_bits = _args.tolerance(fn, "near", near)
    if isinstance(near, bool):
        raise ValueError(f"{fn}: near must be a number, got {near}")
    fr, _ = _number(fn, "far", far)
    st, st_bits = _positive(fn, "step", vs if step is None else step)
    mw, mw_bits = _number(fn, "min_weight", min_weight)
    if not math.isfinite(fr) or fr < nr:
        raise ValueError(f"{fn}: far must be finite and not below near, got near={near} far={far}")
    K = int(math.floor((fr - nr) / st)) + 1
    if K > _MAX_SAMPLES:
        raise ValueError(f"{fn}: {K} samples between near and far; at most {_MAX_SAMPLES} (a larger step, or a shorter range)")
    if color_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{fn}: color_dtype must be torch.uint8 or torch.float32, got {color_dtype}")
    if return_color and volume.color is None:
        raise ValueError(f"{fn}: return_color needs a volume with colours (volume.color is None)")
    _args.max_elems(fn, f"grid={Nz}x{Ny}x{Nx} size={Ho}x{Wo}", Nx * Ny * Nz, 3 * Ho * Wo)
    dev = volume.tsdf.device
    _args.one_gpu(fn, dev, T, rays, *_args.prepared_rows(camera))
    with torch.cuda.device(dev):
        cam = prepare_camera(camera, B, dev)
        if rays is None and _args.n_iterative(cam):                # not fused: the radial loop ends on a maximum over the image
            rays = unproject_camera(None, cam, normalize=True, image_shape=(Ho, Wo))
        return dict(B=B, Nz=Nz, Ny=Ny, Nx=Nx, Ho=Ho, Wo=Wo, vs=vs, vs_bits=vs_bits, near=nr, near_bits=nr_bits, step=st, step_bits=st_bits,
                    min_weight=mw, min_weight_bits=mw_bits, K=K, dev=dev, cam=cam, rays=None if rays is None else rays.contiguous(),
                    Ti=None if T is None else invert_rigid(T.contiguous()).contiguous())


def _render_result(B, Ho, Wo, depth, valid, points, normals, color):
    res = (depth.view(B, 1, Ho, Wo), valid.view(B, 1, Ho, Wo).view(torch.bool))
    return res + tuple(x.view(B, 3, Ho, Wo) for x in (points, normals, color) if x is not None)


def tsdf_render(volume: TsdfVolume, camera, size, transforms: Optional[torch.Tensor] = None, *, rays: Optional[torch.Tensor] = None,
                near: float, far: float, step: Optional[float] = None, min_weight: float = 1.0, return_points: bool = False,
                return_normals: bool = False, return_color: bool = False, color_dtype: torch.dtype = torch.uint8):
    """A TsdfVolume seen from a camera: every pixel's ray marched through the volume to the first surface it meets from the front, the
    whole batch in one launch (KinectFusion's surface prediction; dense and occlusion-correct where render_depth's splat leaves holes).

    volume      a TsdfVolume of B grids (contiguous fp32 on the GPU, else ValueError), from tsdf_integrate.
    camera      as gtpoints.prepare_camera takes it for B images; a PreparedCamera is accepted and nothing is copied from the host then.
    size        (Ho, Wo) of the rendered images.
    transforms  fp32 [4,4], [3,4] or [B,4,4] / [B,3,4]: VOLUME (world) TO CAMERA coordinates, tsdf_integrate's convention, so the
                matrix that integrated a view renders it.  Inverted with consistency.invert_rigid before the launch.  None: identity.
    rays        fp32 [B,3,Ho,Wo]: the pixels' directions in the camera frame, used as they are in place of the camera's; the camera then
                only selects the depth (the distance for Spherical, z otherwise).
    near, far, step   the samples t_k = near + k * step, k = 0 .. K-1, K = floor((far - near) / step) + 1 from the fp32 values; step
                defaults to volume.voxel_size.  ValueError when far < near or K > 16384.
    min_weight  a sample counts only where all eight voxels around it have at least this weight.

    Sample k of a pixel with direction d (the camera's normalised ray of the pixel centre): p = T^-1 (t_k d); g = (p - origin) /
    voxel_size - 0.5 per axis; in the grid when 0 <= g <= N - 1 on every axis; its value s the trilinear interpolant of the eight voxels
    around it, x then y then z; valid when in the grid, the weights pass and s is not a NaN.  Two valid samples in a row with
    !(s_prev < 0) and s < 0 are the hit; with s_prev < 0 and !(s < 0) the ray ends without one (the surface seen from behind).  At the hit
    al = s_prev / (s_prev - s), t* = t_(k-1) + al * (t_k - t_(k-1)), the point q* = t* d and the depth the camera model's depth of q*.

    ->  depth fp32 [B,1,Ho,Wo], valid bool [B,1,Ho,Wo] (hit and depth > 0; every output is exactly 0 where not valid); then, when asked,
        points   fp32 [B,3,Ho,Wo]: q*, in the camera frame
        normals  fp32 [B,3,Ho,Wo]: the gradient of the interpolant at both samples blended with al, rotated into the camera frame,
                 normalised and turned towards the viewer (a fronto-parallel plane gives (0, 0, -1), as normals_from_points); 0 where
                 it is zero or not finite
        color    [B,3,Ho,Wo] color_dtype: the trilinear colours of both samples blended with al; torch.uint8 rounds half to even.

    One launch (csrc/tsdf_render.hip; the arithmetic of a ray is csrc/tsdf_ray.h).  With an OPENCV or Fisheye624 member in the camera,
    whose radial loop ends on a maximum over the whole image, the rays of the batch come from unproject_camera(None, camera,
    normalize=True, image_shape=size) first, the route warp_camera takes.  Stream-ordered, nothing synchronises, no workspace: captures
    into a graph (with a PreparedCamera).  The HIP kernel is the only implementation: CPU tensors raise."""
    fn = "tsdf_render"
    a = _render_arguments(fn, volume, camera, size, transforms, rays, near, far, step, min_weight, return_color, color_dtype)
    B, Ho, Wo, dev = a["B"], a["Ho"], a["Wo"], a["dev"]
    with torch.cuda.device(dev):
        depth = torch.empty((B, Ho, Wo), device=dev, dtype=torch.float32)
        valid = torch.empty((B, Ho, Wo), device=dev, dtype=torch.uint8)
        points = torch.empty((B, 3, Ho, Wo), device=dev, dtype=torch.float32) if return_points else None
        normals = torch.empty((B, 3, Ho, Wo), device=dev, dtype=torch.float32) if return_normals else None
        color = torch.empty((B, 3, Ho, Wo), device=dev, dtype=color_dtype) if return_color else None
        Ti = a["Ti"]
        desc = mk(_lib.UdTsdfRender, tsdf=volume.tsdf, weight=volume.weight, color=volume.color, origin=volume.origin, T=Ti, params=a["cam"].params,
                  rays=a["rays"], depth=depth, valid=valid, points=points, normals=normals, color_out=color, B=B, Ho=Ho, Wo=Wo, Nx=a["Nx"],
                  Ny=a["Ny"], Nz=a["Nz"], nT=0 if Ti is None else Ti.shape[0], n_origin=volume.origin.shape[0], K=a["K"],
                  color_f32=int(color_dtype == torch.float32), voxel_size_bits=a["vs_bits"], near_bits=a["near_bits"],
                  step_bits=a["step_bits"], min_weight_bits=a["min_weight_bits"], **_RENDER_OPTIONS)
        _args.set_models(desc.model, a["cam"])
        check(_lib.lib.ud_tsdf_render(desc, cur_stream()), "ud_tsdf_render")
    return _render_result(B, Ho, Wo, depth, valid, points, normals, color)


def _sample_t(near, step, k):
    """t_k = near + (float)k * step with both operations rounded to fp32, as a Python float"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)             # noqa: E731
    return float(f(near) + f(float(k)) * f(step))


def _lerp(a, b, f):
    return a + f * (b - a)


def _render_compose(a, volume, return_points, return_normals, return_color, color_dtype):
    B, Ho, Wo, dev = a["B"], a["Ho"], a["Wo"], a["dev"]
    Nx, Ny, Nz = a["Nx"], a["Ny"], a["Nz"]
    hw, n = Ho * Wo, Nx * Ny * Nz
    d = a["rays"] if a["rays"] is not None else unproject_camera(None, a["cam"], normalize=True, image_shape=(Ho, Wo))
    dx, dy, dz = (c.contiguous() for c in d.reshape(B, 3, hw).unbind(1))
    T = None if a["Ti"] is None else [a["Ti"][:, r, c].reshape(-1, 1) for r in range(3) for c in range(4)]
    o = [volume.origin[:, k].reshape(-1, 1) for k in range(3)]
    vs = torch.full((), a["vs"], device=dev)                       # a divisor as a device tensor: a division, not a reciprocal
    tsdf, weight = volume.tsdf.reshape(B, n), volume.weight.reshape(B, n)
    color = volume.color.reshape(B, 3, n) if return_color else None
    detail = return_normals or return_color
    mw = a["min_weight"]

    def sample(t):
        """-> valid, s, the eight distances, (fx, fy, fz), the eight indices"""
        x, y, z = dx * t, dy * t, dz * t
        if T is not None:
            x, y, z = (((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3] for r in range(3))
        g = [(p - o[k]) / vs - 0.5 for k, p in enumerate((x, y, z))]
        inside = None
        for gk, N in zip(g, (Nx, Ny, Nz)):
            ok = (gk >= 0) & (gk <= float(N - 1))
            inside = ok if inside is None else inside & ok
        lo, up, f = [], [], []
        for gk, N in zip(g, (Nx, Ny, Nz)):
            gs = torch.where(inside, gk, torch.zeros_like(gk))     # no float becomes an index before it is known to be safe
            i = torch.floor(gs).long().clamp(max=N - 2).clamp(min=0)
            lo.append(i)
            up.append((i + 1).clamp(max=N - 1))
            f.append(gs - i.float())
        idx = [((iz * Ny + iy) * Nx + ix) for iz in (lo[2], up[2]) for iy in (lo[1], up[1]) for ix in (lo[0], up[0])]
        ok = inside
        for i in idx:
            ok = ok & (torch.gather(weight, 1, i) >= mw)
        v = [torch.gather(tsdf, 1, i) for i in idx]
        s = _tri(v, f)
        return ok & ~torch.isnan(s), s, v, f, idx

    def _tri(v, f):
        c00, c10, c01, c11 = _lerp(v[0], v[1], f[0]), _lerp(v[2], v[3], f[0]), _lerp(v[4], v[5], f[0]), _lerp(v[6], v[7], f[0])
        return _lerp(_lerp(c00, c10, f[1]), _lerp(c01, c11, f[1]), f[2])

    def details(v, f, idx):
        g = [_lerp(_lerp(v[1] - v[0], v[3] - v[2], f[1]), _lerp(v[5] - v[4], v[7] - v[6], f[1]), f[2]),
             _lerp(_lerp(v[2] - v[0], v[3] - v[1], f[0]), _lerp(v[6] - v[4], v[7] - v[5], f[0]), f[2]),
             _lerp(_lerp(v[4] - v[0], v[5] - v[1], f[0]), _lerp(v[6] - v[2], v[7] - v[3], f[0]), f[1])] if return_normals else None
        c = [_tri([torch.gather(color[:, k], 1, i) for i in idx], f) for k in range(3)] if return_color else None
        return g, c

    zero = torch.zeros((B, hw), device=dev)
    false = torch.zeros((B, hw), device=dev, dtype=torch.bool)
    have, done, hit, sp = false, false, false, zero
    al, ts = zero, zero
    G = [zero] * 3 if return_normals else None
    C = [zero] * 3 if return_color else None
    prev = None
    for k in range(a["K"]):
        t1 = _sample_t(a["near"], a["step"], k)
        valid, s, v, f, idx = sample(t1)
        cur = details(v, f, idx) if detail else None
        both = valid & have & ~done
        now = both & ~(sp < 0) & (s < 0)
        if k > 0:
            t0 = _sample_t(a["near"], a["step"], k - 1)
            alk = sp / (sp - s)
            al = torch.where(now, alk, al)
            ts = torch.where(now, t0 + alk * (t1 - t0), ts)            # t1 - t0: exact in double, rounded to fp32 by the multiply
            if return_normals:
                G = [torch.where(now, prev[0][j] + alk * (cur[0][j] - prev[0][j]), G[j]) for j in range(3)]
            if return_color:
                C = [torch.where(now, prev[1][j] + alk * (cur[1][j] - prev[1][j]), C[j]) for j in range(3)]
        hit = hit | now
        done = done | now | (both & (sp < 0) & ~(s < 0))
        have, sp, prev = valid, s, cur
    x, y, z = ts * dx, ts * dy, ts * dz
    spherical = torch.tensor([m == 3 for m in a["cam"].models], device=dev).reshape(B, 1)
    dep = torch.where(spherical, torch.sqrt(x * x + y * y + z * z), z)
    valid = hit & (dep > 0)
    out = lambda t: torch.where(valid, t, zero)                    # noqa: E731
    depth = out(dep)
    points = torch.stack([out(x), out(y), out(z)], dim=1) if return_points else None
    normals = col = None
    if return_normals:
        nx, ny, nz = G
        if T is not None:
            nx, ny, nz = ((T[c] * G[0] + T[4 + c] * G[1]) + T[8 + c] * G[2] for c in range(3))
        finite = torch.isfinite(nx) & torch.isfinite(ny) & torch.isfinite(nz)
        m = torch.maximum(torch.maximum(nx.abs(), ny.abs()), nz.abs())
        good = finite & (m > 0)
        nx, ny, nz = nx / m, ny / m, nz / m
        length = torch.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / length, ny / length, nz / length
        flip = ((nx * x + ny * y) + nz * z) > 0
        nx, ny, nz = (torch.where(flip, -c, c) for c in (nx, ny, nz))
        good = good & torch.isfinite(nx) & torch.isfinite(ny) & torch.isfinite(nz) & valid
        normals = torch.stack([torch.where(good, c, zero) for c in (nx, ny, nz)], dim=1)
    if return_color:
        col = torch.stack([out(c) for c in C], dim=1)
        if color_dtype == torch.uint8:
            col = torch.where(torch.isnan(col), torch.zeros_like(col), torch.round(col).clamp(0, 255)).to(torch.uint8)
    return _render_result(B, Ho, Wo, depth, valid.view(torch.uint8), points, normals, col)


def tsdf_render_composition(volume: TsdfVolume, camera, size, transforms: Optional[torch.Tensor] = None, *, rays: Optional[torch.Tensor] = None,
                            near: float, far: float, step: Optional[float] = None, min_weight: float = 1.0, return_points: bool = False,
                            return_normals: bool = False, return_color: bool = False, color_dtype: torch.dtype = torch.uint8):
    """tsdf_render's definition spelled in torch: arguments and results as there.  The directions come from unproject_camera(None, camera,
    normalize=True, image_shape=size) (or `rays`); then a Python loop over the K samples, each a few hundred launches over all pixels:
    the rigid motion and the grid coordinates element-wise, torch.gather for the eight weights and distances (and colours), torch.where
    for the scan's state and the crossing.  Every sample of every ray is visited (the full scan).  This is the second oracle of the fused
    kernel's tests, after the numpy restatement, and the counterpart of its benchmark."""
    a = _render_arguments("tsdf_render_composition", volume, camera, size, transforms, rays, near, far, step, min_weight, return_color, color_dtype)
    with torch.cuda.device(a["dev"]):
        return _render_compose(a, volume, return_points, return_normals, return_color, color_dtype)
