"""Multi-view depth consistency and fusion: the forward-backward geometric filter of multi-view stereo for the depths of several frames,
their cameras and their poses -- what to run before fusing frames into one cloud (pack_points, save_ply).

    depth_consistency(depth, camera, src_depths, src_cameras, transforms, ...)     one ud_depth_consistency call (csrc/consistency.hip)
    depth_consistency_composition(...)      the same definition spelled with warp_camera, unproject_camera, project_camera and torch
    invert_rigid(T)                         [R^T | -(R^T t)] in fp32, the inverse both of them use

For every pixel of the reference view and every neighbour view: move the pixel's point into the view, read the view's depth there, lift
that sample back through the view's camera, bring it home, project it through the reference camera; the view agrees when the point lands
within px_tol pixels of where it started and its depth within rel_tol of the reference depth.  The fused kernel keeps the reference
point in registers across all views and every intermediate map out of memory; every output has the bits the composition gives.  The HIP
kernel is the only implementation of the fused form: CPU tensors raise."""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence

import torch

from . import _args, _lib
from .gtpoints import PreparedCamera, prepare_camera
from .ops import check, cur_stream, mk
from .reproject import project_camera
from .unproject import unproject_camera
from .warp import warp_camera


def invert_rigid(T: torch.Tensor) -> torch.Tensor:
    """The inverse [R^T | -(R^T t)] of rigid motions T = [R | t], fp32 [...,3,4] or [...,4,4] (the last row of a 4x4 is copied), in the
    shape of the input.  Element-wise fp32 multiplies and adds in a fixed order, no matmul, so that the fused kernel and the composition
    receive the same bits on every device: row i of the new translation is -((R[0,i] * t[0] + R[1,i] * t[1]) + R[2,i] * t[2])."""
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float32 or T.ndim < 2 or tuple(T.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError("invert_rigid: T must be fp32 [...,3,4] or [...,4,4]")
    R, t = T[..., :3, :3], T[..., :3, 3]
    Rt = R.transpose(-1, -2)
    ti = -((Rt[..., :, 0] * t[..., 0:1] + Rt[..., :, 1] * t[..., 1:2]) + Rt[..., :, 2] * t[..., 2:3])
    out = T.clone()
    out[..., :3, :3] = Rt
    out[..., :3, 3] = ti
    return out


def _arguments(fn, depth, camera, src_depths, src_cameras, transforms, px_tol, rel_tol, min_views, valid_in, src_masks):
    """every check both functions share -> the sizes, the tolerances and the tensors in the layout of the descriptor"""
    B, H, W = _args.depth_map(fn, "depth", depth)
    _args.float_tensor(fn, "src_depths", src_depths)
    if src_depths.ndim != 4 or min(src_depths.shape) == 0 or src_depths.shape[0] != B:
        raise ValueError(f"{fn}: src_depths must be [B,V,Hs,Ws] with B = {B}, non-empty, got {tuple(src_depths.shape)}")
    V, Hs, Ws = src_depths.shape[1:]
    if V > 255 or B * V > _lib.UD_RECON_MAX_B:
        raise ValueError(f"{fn}: src_depths: at most 255 views and {_lib.UD_RECON_MAX_B} image-view pairs per call, got B={B} V={V}")
    _args.max_elems(fn, f"V={V} source={Hs}x{Ws} reference={H}x{W}", H * W, V * Hs * Ws)
    if isinstance(src_cameras, (torch.Tensor, PreparedCamera)) or not isinstance(src_cameras, Sequence) or len(src_cameras) != V:
        raise ValueError(f"{fn}: src_cameras must be a sequence of {V} cameras, one per view")
    for name, cam in [("camera", camera)] + [(f"src_cameras[{v}]", c) for v, c in enumerate(src_cameras)]:
        _args.batch_of(fn, name, _args.n_cameras(cam), B, shared=not isinstance(cam, PreparedCamera))
    shapes = ((V, 4, 4), (V, 3, 4), (B, V, 4, 4), (B, V, 3, 4))
    if not isinstance(transforms, torch.Tensor) or transforms.dtype != torch.float32 or tuple(transforms.shape) not in shapes:
        raise ValueError(f"{fn}: transforms must be fp32 [{V},4,4], [{B},{V},4,4] or the 3x4 forms of either")
    px, px_bits = _args.tolerance(fn, "px_tol", px_tol)
    rel, rel_bits = _args.tolerance(fn, "rel_tol", rel_tol)
    if isinstance(min_views, bool) or not isinstance(min_views, int) or not 0 <= min_views <= V:
        raise ValueError(f"{fn}: min_views must be an integer in 0 .. {V}, got {min_views!r}")
    if valid_in is not None:
        _args.image_map(fn, "valid_in", valid_in, H, W, mask=True, B=B, shared=False)
    if src_masks is not None:
        _args.mask_tensor(fn, "src_masks", src_masks)
        if tuple(src_masks.shape) != (B, V, Hs, Ws):
            raise ValueError(f"{fn}: src_masks {tuple(src_masks.shape)} is not [{B},{V},{Hs},{Ws}]")
    dev = depth.device
    _args.one_gpu(fn, dev, src_depths, transforms, valid_in, src_masks, *_args.prepared_rows(camera, *src_cameras))
    with torch.cuda.device(dev):
        a = dict(B=B, V=V, H=H, W=W, Hs=Hs, Ws=Ws, px=px, px_bits=px_bits, rel=rel, rel_bits=rel_bits, min_views=min_views, dev=dev)
        a["cam"] = prepare_camera(camera, B, dev)
        a["cams"] = [prepare_camera(c, B, dev) for c in src_cameras]
        a["depth"] = depth.reshape(B, H, W).float().contiguous()
        a["src"] = src_depths.float().contiguous()
        a["T"] = transforms[..., :3, :].reshape(-1, V, 3, 4).contiguous()
        a["Tinv"] = invert_rigid(a["T"])
        a["vin"] = None if valid_in is None else valid_in.reshape(B, H, W).contiguous().view(torch.uint8)
        a["masks"] = None if src_masks is None else src_masks.contiguous().view(torch.uint8)
    a["iterative"] = _args.n_iterative(a["cam"], *a["cams"]) > 0
    return a


def _results(fused, count, mask, cons, epx, erel, return_views, return_errors):
    res = (fused, count, mask)
    if return_views:
        res += (cons,)
    if return_errors:
        res += (epx, erel)
    return res


def _compose(a, return_views, return_errors):
    B, V, H, W, dev = a["B"], a["V"], a["H"], a["W"], a["dev"]
    depth = a["depth"][:, None]                                                     # [B,1,H,W]
    ref_ok = depth > 0
    if a["vin"] is not None:
        ref_ok = ref_ok & a["vin"][:, None].bool()
    cu = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5).view(1, 1, 1, W)
    cw = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5).view(1, 1, H, 1)
    try:
        tol2 = struct.unpack("<f", struct.pack("<f", a["px"] * a["px"]))[0]         # the product of two fp32 values rounded once to fp32
    except OverflowError:
        tol2 = math.inf                                                             # as the fp32 product overflows
    bar = depth * a["rel"]
    total, count = depth.clone(), torch.zeros((B, 1, H, W), device=dev, dtype=torch.uint8)
    zero = torch.zeros((), device=dev, dtype=torch.float32)
    cons, epx, erel = [], [], []
    for v in range(V):
        sd = a["src"][:, v:v + 1]
        m = sd > 0
        if a["masks"] is not None:
            m = m & a["masks"][:, v:v + 1].bool()
        T, Tinv = a["T"][:, v].contiguous(), a["Tinv"][:, v].contiguous()            # [nT,3,4]
        ds, sampled, uv = warp_camera(sd, depth=depth, camera=a["cam"], src_camera=a["cams"][v], transform=T, src_mask=m,
                                      valid_in=a["vin"], normalize=True, return_mask=True, return_uv=True)
        lifted = unproject_camera(uv, a["cams"][v], depth=ds)
        uv2, inside, dback = project_camera(lifted, a["cam"], (H, W), transform=Tinv)
        dback, inside = dback[:, None], inside[:, None]
        du, dv = uv2[:, 0:1] - cu, uv2[:, 1:2] - cw
        e2 = du * du + dv * dv
        diff = (dback - depth).abs()
        c = sampled & inside & (dback > 0) & (e2 <= tol2) & (diff <= bar)
        total = torch.where(c, total + dback, total)
        count = count + c.to(torch.uint8)
        if return_views:
            cons.append(c)
        if return_errors:
            epx.append(torch.where(sampled, e2.sqrt(), zero))
            erel.append(torch.where(sampled, diff / depth, zero))
    fused = torch.where(ref_ok, total / (count.float() + 1.0), zero)
    mask = ref_ok & (count >= a["min_views"])
    cat = lambda parts: torch.cat(parts, dim=1) if parts else None                  # noqa: E731
    return _results(fused, count, mask, cat(cons), cat(epx), cat(erel), return_views, return_errors)


def depth_consistency_composition(depth: torch.Tensor, camera, src_depths: torch.Tensor, src_cameras, transforms: torch.Tensor, *,
                                  px_tol: float = 1.0, rel_tol: float = 0.01, min_views: int = 1, valid_in: Optional[torch.Tensor] = None,
                                  src_masks: Optional[torch.Tensor] = None, return_views: bool = False, return_errors: bool = False):
    """depth_consistency's definition spelled with the separate calls, in a loop over the views: arguments and results as there, any of
    the six camera models on either side.  Per view: warp_camera(src_depths[:, v], depth=depth, camera=camera, src_camera=src_cameras[v],
    transform=transforms[v], src_mask=(src_depths[:, v] > 0) & src_masks[:, v], normalize=True, return_mask=True, return_uv=True) gives
    the sample, its validity and (u, v); unproject_camera(uv, src_cameras[v], depth=sample) lifts it; project_camera(lifted, camera,
    (H, W), transform=invert_rigid(transforms)[v]) brings it home; torch element-wise arithmetic, every operation a launch of its own,
    forms du, dv, e2 = du * du + dv * dv, diff = |dback - depth|, the decision, the running sum and the count.  Three library launches and
    about 25 element-wise ones per view.  This is the oracle of the fused kernel's tests and what depth_consistency runs for OPENCV
    and Fisheye624 cameras."""
    a = _arguments("depth_consistency_composition", depth, camera, src_depths, src_cameras, transforms, px_tol, rel_tol, min_views, valid_in,
                   src_masks)
    with torch.cuda.device(a["dev"]):
        return _compose(a, return_views, return_errors)


def depth_consistency(depth: torch.Tensor, camera, src_depths: torch.Tensor, src_cameras, transforms: torch.Tensor, *, px_tol: float = 1.0,
                      rel_tol: float = 0.01, min_views: int = 1, valid_in: Optional[torch.Tensor] = None,
                      src_masks: Optional[torch.Tensor] = None, return_views: bool = False, return_errors: bool = False):
    """The forward-backward depth check of a reference view against V neighbour views and the fused depth, the whole batch in one launch.

    depth, camera  the reference view's depth [B,1,H,W] or [B,H,W] (any float dtype, converted to contiguous fp32) and its camera.
    src_depths     the neighbour views' depths [B,V,Hs,Ws] (any float dtype), one size for all views.
    src_cameras    a sequence of V cameras, one per view.  Cameras are as gtpoints.prepare_camera takes them for B images; a PreparedCamera
                   is accepted and nothing is copied from the host then (graph capture).
    transforms     fp32 [V,4,4] or [B,V,4,4] (or the 3x4 forms): reference-camera to view-v-camera coordinates.  The way back is
                   invert_rigid(transforms).
    px_tol, rel_tol   the reprojection tolerance in pixels and the relative depth tolerance, rounded to fp32.
    min_views      mask needs at least this many agreeing views, 0 .. V.
    valid_in       bool / uint8 [B,1,H,W] / [B,H,W]: reference pixels with 0 are not ok.
    src_masks      bool / uint8 [B,V,Hs,Ws]: view pixels with 0 contribute to no sample.

    Reference pixel (x, y): ref_ok = valid_in & (depth > 0), false for a NaN; P = the camera's reconstruct at the pixel centre.  View v:
    Q = T P, (u, v) its projection through the view's camera; the view's depth sampled there bilinearly from the taps with a depth > 0
    (warp_camera's normalised form, valid as there); that sample reconstructed through the view's camera, moved by the inverse and
    projected through the reference camera to (u', v') with depth dback.  The view is consistent when the sample is valid, (u', v') is
    inside the image, dback > 0, (u' - x - .5)^2 + (v' - y - .5)^2 <= px_tol^2 and |dback - depth| <= rel_tol * depth, all in fp32,
    false whenever anything is a NaN.

    ->  fused  fp32 [B,1,H,W]   (depth + the dback of the consistent views, in view order) / (count + 1); 0 where ref_ok is False
        count  uint8 [B,1,H,W]  the consistent views
        mask   bool [B,1,H,W]   ref_ok & (count >= min_views)
        consistent  bool [B,V,H,W] (return_views=True)
        err_px, err_rel  fp32 [B,V,H,W] (return_errors=True): the reprojection error in pixels and |dback - depth| / depth, 0 where the
                   sample is not valid

    One launch, plus the few small ones that stack the views' parameter rows and invert the transforms.  Stream-ordered, nothing
    synchronises, no workspace: captures into a graph (with PreparedCamera cameras).  With an OPENCV or Fisheye624 member in any camera,
    whose unprojection ends on a maximum over the whole image, the call runs depth_consistency_composition instead: three library
    launches and about 25 element-wise ones per view (more for such a reference, see warp_camera)."""
    fn = "depth_consistency"
    a = _arguments(fn, depth, camera, src_depths, src_cameras, transforms, px_tol, rel_tol, min_views, valid_in, src_masks)
    B, V, H, W, dev = a["B"], a["V"], a["H"], a["W"], a["dev"]
    with torch.cuda.device(dev):
        if a["iterative"]:
            return _compose(a, return_views, return_errors)
        params_src = torch.stack([c.params for c in a["cams"]])                       # [V,B,16]
        fused = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
        count = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8)
        mask = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8)
        cons = torch.empty((B, V, H, W), device=dev, dtype=torch.uint8) if return_views else None
        epx = torch.empty((B, V, H, W), device=dev, dtype=torch.float32) if return_errors else None
        erel = torch.empty((B, V, H, W), device=dev, dtype=torch.float32) if return_errors else None
        desc = mk(_lib.UdDepthConsistency, depth=a["depth"], params_ref=a["cam"].params, valid_in=a["vin"], src_depth=a["src"],
                  src_mask=a["masks"], params_src=params_src, T=a["T"], Tinv=a["Tinv"], fused=fused, count=count, mask=mask, consistent=cons,
                  err_px=epx, err_rel=erel, B=B, V=V, H=H, W=W, Hs=a["Hs"], Ws=a["Ws"], nT=a["T"].shape[0], min_views=a["min_views"],
                  px_tol_bits=a["px_bits"], rel_tol_bits=a["rel_bits"])
        _args.set_models(desc.model_ref, a["cam"])
        for v in range(V):
            _args.set_models(desc.model_src, a["cams"][v], v * B)
        check(_lib.lib.ud_depth_consistency(desc, cur_stream()), "ud_depth_consistency")
    return _results(fused, count, mask.view(torch.bool), None if cons is None else cons.view(torch.bool), epx, erel, return_views, return_errors)
