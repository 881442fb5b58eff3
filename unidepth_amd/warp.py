"""Backward warping through the camera models: a second view's image, depth or features fetched at every pixel of a first view, from the
first view's depth (or point map), its camera, a relative pose and the second view's camera, with a visibility test -- view synthesis for
photometric checks, multi-view depth consistency, label transfer between a fisheye and a pinhole rig.

    warp_camera(src, depth=..., camera=..., src_camera=..., transform=...)      one ud_warp_camera call (csrc/warp.hip)

It is unproject_camera, project_camera and remap (and a second remap of the source's depth) fused into one launch with one thread per
destination pixel: the point map, the coordinate map, the inside mask and the projected depth never reach memory, and every output has
the bits the separate calls give.  The HIP kernel is the only implementation: CPU tensors raise."""
from __future__ import annotations

from typing import Optional

import torch

from . import _args, _lib
from .gtpoints import PreparedCamera, prepare_camera
from .ops import check, cur_stream, mk
from .remap import _MODES, _PADDINGS
from .unproject import unproject_camera


def warp_camera(src: torch.Tensor, *, depth: Optional[torch.Tensor] = None, camera=None, points: Optional[torch.Tensor] = None, src_camera,
                transform: Optional[torch.Tensor] = None, mode: str = "bilinear", padding: str = "zeros",
                src_mask: Optional[torch.Tensor] = None, valid_in: Optional[torch.Tensor] = None, normalize: bool = False,
                out_dtype: Optional[torch.dtype] = None, src_depth: Optional[torch.Tensor] = None, occlusion_tol: Optional[float] = None,
                return_mask: bool = False, return_uv: bool = False, return_depth: bool = False):
    """The maps `src` of a source view fetched at every pixel of a destination view, the whole batch in one launch.

    src            [B,C,Hs,Ws] (or [1,C,Hs,Ws], shared), any float dtype (converted to contiguous fp32) or uint8: remap's src.
    depth, camera  the destination view's depth [B,1,Ho,Wo] or [B,Ho,Wo] (any float dtype) and its camera: the point of a pixel is the
                   camera's reconstruct at the pixel centre, as unproject_camera(None, camera, depth=depth, image_shape=(Ho, Wo)).
    points         or the points themselves, [B,3,Ho,Wo] (infer()'s `points`), in the destination camera's frame.  Exactly one of
                   depth (+ camera) and points.
    src_camera     the source view's camera.  Cameras are as gtpoints.prepare_camera takes them, any of the six models, one per image; a
                   PreparedCamera is accepted and nothing is copied from the host then (graph capture).
    transform      fp32 [3,4] / [4,4] (or [1,..] / [B,..]) as project_camera takes it: destination-camera to source-camera coordinates.
    mode, padding, src_mask, normalize, out_dtype: remap's, applied at (u, v) = project_camera's coordinates of the moved points.
    valid_in       bool / uint8 [B,1,Ho,Wo] / [B,Ho,Wo] (a batch of 1 is shared): destination pixels with 0 sample nothing.
    src_depth, occlusion_tol   the source view's depth [B or 1,1,Hs,Ws] (any float dtype) and a relative tolerance, together or not at
                   all: the visibility test below.

    A pixel samples where  cv = inside & (proj_depth > 0) [& valid_in] [& (depth > 0)]  holds -- project_camera's `inside` and depth of
    the moved point; the last term in the depth form only, false for a NaN.  The destination model's unprojection mask is deliberately
    NOT part of it, so the depth form and the points form agree: pass unproject_camera(..., return_mask=True)'s mask as valid_in where
    it is wanted.

    ->  out [B,C,Ho,Wo]: remap(src, uv, coord_valid=cv, ...), 0 where cv is False or a coordinate is not finite; then, in this order,
        valid      bool [B,1,Ho,Wo] (return_mask=True): remap's -- cv, finite coordinates inside [0, Ws] x [0, Hs], a tap of non-zero weight
        visible    bool [B,1,Ho,Wo] (when src_depth is given): src_depth sampled at the same taps with the same mode and padding (a tap
                   contributes only if its src_depth > 0 and its src_mask is not 0; bilinear in the normalised form) is valid and
                   |sampled - proj_depth| <= occlusion_tol * proj_depth in fp32; False for a NaN
        uv         fp32 [B,2,Ho,Wo] (return_uv=True): project_camera's coordinates, every pixel
        proj_depth fp32 [B,Ho,Wo] (return_depth=True): project_camera's depth, the source model's (z, or the distance for Spherical)
        A tuple only when there is more than one.

    Values are RESAMPLED, not converted, as undistort: a depth map fetched from a Spherical source keeps its numbers.

    One launch.  With an OPENCV or Fisheye624 member in the destination camera, whose radial loop ends on a maximum over the whole image,
    the points of the whole batch come from unproject_camera first and `depth > 0` is ANDed into valid_in: five launches (three of
    unproject_camera, one comparison, the warp), six with a valid_in.  Stream-ordered, nothing synchronises, no workspace: captures into
    a graph (with PreparedCamera cameras)."""
    fn = "warp_camera"
    if mode not in _MODES:
        raise ValueError(f"{fn}: mode must be one of {tuple(_MODES)}, got {mode!r}")
    if padding not in _PADDINGS:
        raise ValueError(f"{fn}: padding must be one of {tuple(_PADDINGS)}, got {padding!r}")
    if not isinstance(src, torch.Tensor) or not (src.is_floating_point() or src.dtype == torch.uint8):
        raise ValueError(f"{fn}: src must be a float or uint8 tensor, got {getattr(src, 'dtype', type(src).__name__)}")
    if src.ndim != 4 or min(src.shape) == 0:
        raise ValueError(f"{fn}: src must be [B,C,Hs,Ws] (B or 1 images), non-empty, got {tuple(src.shape)}")
    sb, Cc, Hs, Ws = src.shape
    src_u8 = src.dtype == torch.uint8
    if out_dtype is None:
        out_dtype = torch.uint8 if src_u8 else torch.float32
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{fn}: out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
    if out_dtype == torch.uint8 and not src_u8:
        raise ValueError(f"{fn}: out_dtype: a uint8 output needs a uint8 source, got {src.dtype}")
    if (depth is None) == (points is None):
        raise ValueError(f"{fn}: exactly one of depth (with camera) and points must be given")
    if depth is not None:
        if camera is None:
            raise ValueError(f"{fn}: depth needs camera, the destination view's camera")
        B, Ho, Wo = _args.depth_map(fn, "depth", depth)
    else:
        if camera is not None:
            raise ValueError(f"{fn}: camera goes with depth; points are already in the destination camera's frame")
        B, Ho, Wo = _args.point_map(fn, "points", points)
    n = Ho * Wo
    sizes = {"src": sb}
    if src_mask is not None:
        sizes["src_mask"] = _args.image_map(fn, "src_mask", src_mask, Hs, Ws, mask=True)
    if (src_depth is None) != (occlusion_tol is None):
        raise ValueError(f"{fn}: src_depth and occlusion_tol come together or not at all")
    tol_bits = 0
    if src_depth is not None:
        sizes["src_depth"] = _args.image_map(fn, "src_depth", src_depth, Hs, Ws, mask=False)
        tol_bits = _args.tolerance(fn, "occlusion_tol", occlusion_tol)[1]         # the descriptor carries the fp32's bit pattern
    if valid_in is not None:
        sizes["valid_in"] = _args.image_map(fn, "valid_in", valid_in, Ho, Wo, mask=True)
    for name, cam in (("camera", camera), ("src_camera", src_camera)):
        if cam is not None:
            sizes[name] = _args.n_cameras(cam)
    _args.batches(fn, sizes, B)
    for name, cam in (("camera", camera), ("src_camera", src_camera)):
        if isinstance(cam, PreparedCamera):
            _args.batch_of(fn, name, len(cam), B, shared=False)
    _args.max_images(fn, B)
    _args.max_elems(fn, f"C={Cc} source={Hs}x{Ws} destination={Ho}x{Wo}", n, Cc * n, Cc * Hs * Ws)
    T, nT = _args.rigid(fn, transform, B)
    dev = src.device
    _args.one_gpu(fn, dev, depth, points, src_mask, valid_in, src_depth, T, *_args.prepared_rows(camera, src_camera))
    with torch.cuda.device(dev):
        cam_s = prepare_camera(src_camera, B, dev)
        cam_d = None
        if depth is not None:
            cam_d = prepare_camera(camera, B, dev)
            d = depth.reshape(B, n).float().contiguous()
            if _args.n_iterative(cam_d):                            # not fused: the radial loop ends on a maximum over the image
                points = unproject_camera(None, cam_d, depth=d.view(B, Ho, Wo), image_shape=(Ho, Wo))
                positive = (d > 0).view(B, Ho, Wo)
                valid_in = positive if valid_in is None else positive & valid_in.reshape(-1, Ho, Wo).bool()
                d = cam_d = None
        else:
            d = None
        pts = None if points is None else points.float().contiguous()
        s = src.contiguous() if src_u8 else src.float().contiguous()
        m = None if src_mask is None else src_mask.contiguous().view(torch.uint8)
        sd = None if src_depth is None else src_depth.float().contiguous()
        vin = None
        if valid_in is not None:
            vin = valid_in.reshape(valid_in.shape[0], n)
            vin = (vin.expand(B, n) if vin.shape[0] != B else vin).contiguous().view(torch.uint8)
        out = torch.empty((B, Cc, Ho, Wo), device=dev, dtype=out_dtype)
        valid = torch.empty((B, 1, Ho, Wo), device=dev, dtype=torch.uint8) if return_mask else None
        visible = torch.empty((B, 1, Ho, Wo), device=dev, dtype=torch.uint8) if sd is not None else None
        uv = torch.empty((B, 2, Ho, Wo), device=dev, dtype=torch.float32) if return_uv else None
        pd = torch.empty((B, Ho, Wo), device=dev, dtype=torch.float32) if return_depth else None
        desc = mk(_lib.UdWarpCamera, src=s, src_mask=m, src_depth=sd, points=pts, depth=d, params_dst=None if cam_d is None else cam_d.params,
                  params_src=cam_s.params, T=T, valid_in=vin, out=out, valid=valid, visible=visible, uv=uv, proj_depth=pd,
                  B=B, C=Cc, Ho=Ho, Wo=Wo, Hs=Hs, Ws=Ws, nT=nT, mode=_MODES[mode], padding=_PADDINGS[padding],
                  normalize=int(bool(normalize)), src_u8=int(src_u8), out_u8=int(out_dtype == torch.uint8), src_shared=int(sb == 1),
                  mask_shared=int(m is not None and m.shape[0] == 1), depth_shared=int(sd is not None and sd.shape[0] == 1),
                  tol_bits=tol_bits)
        _args.set_models(desc.model_src, cam_s)
        if cam_d is not None:
            _args.set_models(desc.model_dst, cam_d)
        check(_lib.lib.ud_warp_camera(desc, cur_stream()), "ud_warp_camera")
    res = (out,)
    if return_mask:
        res += (valid.view(torch.bool),)
    if visible is not None:
        res += (visible.view(torch.bool),)
    if return_uv:
        res += (uv,)
    if return_depth:
        res += (pd,)
    return _args.tail(res)
