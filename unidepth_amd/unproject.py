"""Viewing rays at arbitrary image coordinates: the reference's Camera.unproject and Camera.get_rays (unidepth/utils/camera.py) for a
whole batch, one camera model per image, in one ud_camera_unproject call (csrc/unproject.hip).

    unproject_camera(uv, camera, ...)   rays fp32 at the coordinates `uv` (keypoints, sparse returns, another camera's pixel grid),
                                        or at the pixel centres of an image when uv is None; optionally normalised, or scaled by a
                                        depth into points (Camera.reconstruct at those coordinates), with the reference's mask
    get_rays(camera, shapes)            Camera.get_rays: the normalised rays of the pixel grid

With reproject.project_camera this closes the loop: project_camera(unproject_camera(grid, dst_cam), src_cam) is the coordinate map
that undistortion and backward warping sample with.  The HIP kernels are the only implementation: CPU tensors raise."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _args, _lib
from .gtpoints import prepare_camera
from .ops import check, cur_stream, mk


def _unproject(fn, uv, camera, depth, normalize, image_shape, return_mask, batch=None):
    if normalize and depth is not None:
        raise ValueError(f"{fn}: normalize and depth exclude each other (a depth scales the ray the model's reconstruct rule defines)")
    if image_shape is not None:
        H, W = _args.image_shape(fn, image_shape)
    if uv is None:
        if image_shape is None:
            raise ValueError(f"{fn}: uv=None (the identity grid) needs image_shape=(H, W)")
        nb, n, tail, rows, strides = 1, H * W, (H, W), 0, (0, 1, 1)
    else:
        _args.float_tensor(fn, "uv", uv)
        nb, n, tail, rows, strides = _args.layout(fn, "uv", uv, 2)
        if nb == 0:
            raise ValueError(f"{fn}: empty batch")
        if image_shape is None:
            H, W = tail if not rows else (1, 1)                  # read for the identity grid only
    if depth is not None:
        _args.float_tensor(fn, "depth", depth)
        if depth.ndim == 0 or depth.shape[0] == 0 or depth.numel() != depth.shape[0] * n or \
                (depth.ndim > 2 and tuple(depth.shape[-2:]) != tail) or (rows and depth.ndim != 2):
            raise ValueError(f"{fn}: depth {tuple(depth.shape)} does not hold one value for each of the {tail} coordinates of every image")
    sizes = [nb, _args.n_cameras(camera)] + ([depth.shape[0]] if depth is not None else []) + ([int(batch)] if batch is not None else [])
    B = max(sizes)
    if uv is not None:
        _args.batch_of(fn, "uv", nb, B)
    if depth is not None:
        _args.batch_of(fn, "depth", depth.shape[0], B, shared=False)
    _args.max_images(fn, B)
    _args.max_elems(fn, f"B={B} points={n}", n)
    dev = uv.device if uv is not None else depth.device if depth is not None else _args.camera_device(camera)
    if dev.type != "cuda" and uv is None and depth is None and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())         # a host camera object and nothing else: the current GPU
    cam = prepare_camera(camera, B, dev)                                 # raises for a CPU batch
    _args.one_gpu(fn, dev, cam.params, depth)
    with torch.cuda.device(dev):
        src = None if uv is None else uv.float().contiguous()
        if src is not None and nb == 1:
            strides = (0,) + strides[1:]
        d = None if depth is None else depth.reshape(B, n).float().contiguous()
        rays = torch.empty((B, n, 3) if rows else (B, 3) + tail, device=dev, dtype=torch.float32)
        valid = torch.empty((B, n) if rows else (B, 1) + tail, device=dev, dtype=torch.uint8) if return_mask else None
        n_iter = _args.n_iterative(cam)
        nbytes = int(_lib.lib.ud_camera_unproject_work_bytes(B, n_iter))
        work = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        desc = mk(_lib.UdCameraUnproject, uv=src, params=cam.params, depth=d, rays=rays, valid=valid, work=work, work_bytes=nbytes,
                  batch_stride=strides[0], point_stride=strides[1], comp_stride=strides[2], n_points=n, B=B, H=H, W=W,
                  normalize=int(bool(normalize)), rays_rows=rows)
        _args.set_models(desc.model, cam)
        check(_lib.lib.ud_camera_unproject(desc, cur_stream()), "ud_camera_unproject")
    return (rays, valid.view(torch.bool)) if return_mask else rays


def unproject_camera(uv: Optional[torch.Tensor], camera, *, depth: Optional[torch.Tensor] = None, normalize: bool = False,
                     image_shape: Optional[Tuple[int, int]] = None, return_mask: bool = False):
    """Camera.unproject for a batch: the ray of every image coordinate through the camera of its image.

    uv      [B,2,H,W] or [B,N,2] image coordinates (pixel centres at half-integers, as gt_points and project_camera place them); a batch
            of 1 is shared by every image.  Any float dtype and layout: converted to contiguous fp32 first.  None with
            image_shape=(H, W): the pixel centres of an H x W image, never materialised.
    camera  as gtpoints.prepare_camera takes it: an intrinsics tensor, a Pinhole / EUCM / Spherical with 1 or B rows, one OPENCV /
            Fisheye624 / MEI (applied to every image), a BatchCamera of B members, a PreparedCamera, or objects of the reference's classes.
            B is the largest of the batches of uv, depth and the camera.
    ->      rays fp32 in the form of the input, [B,3,H,W] or [B,N,3]: each class's own unproject value, NOT normalised --
                Pinhole ((u - cx) / fx, (v - cy) / fy, 1); EUCM (c mx, c my, max(c mz, 1e-3)); Spherical the unit-sphere direction;
                OPENCV, Fisheye624 (dx, dy, 1); MEI (dx, dy, pz)
            normalize=True: rays / max(|rays|, 1e-4), as Camera.get_rays.
            depth ([B,1,H,W] / [B,H,W] for a planar uv, [B,N] for rows): the class's reconstruct at those coordinates -- Pinhole
            r * max(depth, 0), Spherical r * depth, the others r / max(r.z, 1e-4) * max(depth, 1e-4); with uv=None this is gt_points, bit
            for bit.  normalize and depth exclude each other.
    return_mask=True: (rays, mask), mask bool [B,1,H,W] or [B,N], the reference's unprojection_mask: Pinhole z > 1e-4; EUCM inside the
            model's domain and z > 1e-3 before the clamp (the reference's own EUCM mask is [B,H,W], without the channel axis); True for
            the classes that set none.

    The radial loop of an OPENCV / Fisheye624 image ends on the largest residual over the coordinates THIS call was given for that image
    (the reference: over the tensor its unproject receives), so a coordinate's ray can depend on which others it was sent with; MEI is
    fully per point.  One launch; with an OPENCV / Fisheye624 member two, after a small one that clears the maxima.  Stream-ordered, nothing synchronises; camera objects and host
    tensors are uploaded with one small copy, which a graph capture does not allow: capture with a prepare_camera() result."""
    return _unproject("unproject_camera", uv, camera, depth, normalize, image_shape, return_mask)


def get_rays(camera, shapes):
    """Camera.get_rays: the normalised rays fp32 [B,3,H,W] of the pixel centres, shapes = (B, H, W) or (H, W) (B from the camera)."""
    try:
        shapes = tuple(int(v) for v in shapes)
    except (TypeError, ValueError):
        shapes = ()
    if len(shapes) not in (2, 3) or min(shapes) <= 0:
        raise ValueError("get_rays: shapes must be (B, H, W) or (H, W), positive")
    return _unproject("get_rays", None, camera, None, True, shapes[-2:], False, batch=shapes[0] if len(shapes) == 3 else None)
