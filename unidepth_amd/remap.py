"""Sampling maps at arbitrary image coordinates: what undistortion, backward warping and keypoint look-ups are made of, for a whole
batch in one ud_remap call (csrc/remap.hip), and the reference's Camera.mask_overlap_projection (unidepth/utils/camera.py:132-154) in
one ud_overlap_mask call.

    remap(src, uv, ...)                 the maps `src` at the coordinates `uv`: nearest or bilinear, zeros or border padding, an optional
                                        source mask (holes), an optional validity of the coordinates, the weight-normalised form for
                                        depth maps with holes, and the validity of every result
    undistort(src, src_camera, ...)     maps seen through src_camera resampled into the pixel grid of dst_camera: unproject_camera,
                                        project_camera and remap, nothing else
    overlap_mask(projected)             Camera.mask_overlap_projection for a batch

Coordinates are this project's: pixel centres at half-integers, as gt_points, project_camera and unproject_camera place them; nothing
is converted to grid_sample's normalised ones.  The HIP kernels are the only implementation: CPU tensors raise."""
from __future__ import annotations

import sys
from typing import Optional, Tuple

import torch

from . import _args, _lib
from .cameras import GT_PINHOLE
from .gtpoints import PreparedCamera, prepare_camera
from .ops import check, cur_stream, mk
from .reproject import project_camera
from .unproject import unproject_camera

_MODES = {"nearest": _lib.UD_REMAP_NEAREST, "bilinear": _lib.UD_REMAP_BILINEAR}
_PADDINGS = {"zeros": _lib.UD_REMAP_ZEROS, "border": _lib.UD_REMAP_BORDER}


def remap(src: torch.Tensor, uv: torch.Tensor, *, mode: str = "bilinear", padding: str = "zeros", src_mask: Optional[torch.Tensor] = None,
          coord_valid: Optional[torch.Tensor] = None, normalize: bool = False, out_dtype: Optional[torch.dtype] = None,
          return_mask: bool = False):
    """The maps `src` sampled at the image coordinates `uv`, every image of the batch in one launch.

    src          [B,C,Hs,Ws] (or [1,C,Hs,Ws], shared by every image), any float dtype (converted to contiguous fp32) or uint8, C >= 1.
    uv           [B,2,Ho,Wo] or [B,N,2] as unproject_camera takes it (pixel centres at half-integers; a batch of 1 is shared; any float
                 dtype and layout, converted to contiguous fp32).  The index-space position is x = u - 0.5, y = v - 0.5.
    mode         "nearest": the pixel rint(x), rint(y), ties to even (grid_sample's), the source's bits.
                 "bilinear": floor(x), floor(x) + 1 and the same in y with lx = x - floor(x), hx = 1 - lx:
                 (v00 hx + v01 lx) hy + (v10 hx + v11 lx) ly in fp32, every operation rounded separately.
    padding      "zeros": a tap outside the source contributes 0, F.grid_sample(padding_mode="zeros", align_corners=False);
                 "border": x and y are clamped to [0, Ws - 1], [0, Hs - 1] first.
    src_mask     bool / uint8 [B or 1,1,Hs,Ws] (or [.,Hs,Ws]): a tap whose mask is 0 does not contribute.
    coord_valid  bool / uint8, one per point ([B,1,Ho,Wo] / [B,Ho,Wo] / [B,N]; a batch of 1 is shared): project_camera's `inside` goes
                 here.  A point with 0 gets the value 0.
    normalize    the sum over the contributing taps divided by the sum of their weights, 0 where that is 0: depth maps with holes.
    out_dtype    torch.float32 or torch.uint8 (uint8 sources only: rounded half to even, clamped to [0, 255]); None: float32 for a
                 float source, uint8 for a uint8 one.
    ->           out in the layout of uv, [B,C,Ho,Wo] or [B,N,C]; with return_mask=True (out, valid), valid bool [B,1,Ho,Wo] / [B,N]:
                 coord_valid, both coordinates finite, 0 <= u <= Ws and 0 <= v <= Hs, and at least one tap of non-zero weight
                 contributed.  A NaN or infinite coordinate gives 0 in every channel; a finite coordinate outside the image is sampled
                 as the padding says, with valid False.

    B is the largest of the batches.  Stream-ordered, nothing synchronises, no workspace: captures into a graph."""
    fn = "remap"
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
        raise ValueError(f"{fn}: a uint8 output needs a uint8 source, got {src.dtype}")
    _args.float_tensor(fn, "uv", uv)
    nb, n, tail, rows, strides = _args.layout(fn, "uv", uv, 2)
    if nb == 0 or n == 0:
        raise ValueError(f"{fn}: empty uv {tuple(uv.shape)}")
    sizes = {"src": sb, "uv": nb}
    if src_mask is not None:
        sizes["src_mask"] = _args.image_map(fn, "src_mask", src_mask, Hs, Ws, mask=True)
    if coord_valid is not None:
        sizes["coord_valid"] = _args.per_point(fn, "coord_valid", coord_valid, n, tail, rows)
    B = max(sizes.values())
    _args.batches(fn, sizes, B)
    _args.max_images(fn, B)
    _args.max_elems(fn, f"C={Cc} source={Hs}x{Ws} points={n}", n, Cc * n, Cc * Hs * Ws)
    dev = src.device
    _args.one_gpu(fn, dev, uv, src_mask, coord_valid)
    with torch.cuda.device(dev):
        s = src.contiguous() if src_u8 else src.float().contiguous()
        coords = uv.float().contiguous()
        if nb == 1:
            strides = (0,) + strides[1:]
        m = None if src_mask is None else src_mask.contiguous().view(torch.uint8)
        cv = None
        if coord_valid is not None:
            cv = coord_valid.reshape(coord_valid.shape[0], n)
            cv = (cv.expand(B, n) if cv.shape[0] != B else cv).contiguous().view(torch.uint8)
        out = torch.empty((B, n, Cc) if rows else (B, Cc) + tail, device=dev, dtype=out_dtype)
        valid = torch.empty((B, n) if rows else (B, 1) + tail, device=dev, dtype=torch.uint8) if return_mask else None
        desc = mk(_lib.UdRemap, src=s, src_mask=m, uv=coords, coord_valid=cv, out=out, valid=valid, batch_stride=strides[0],
                  point_stride=strides[1], comp_stride=strides[2], n_points=n, B=B, C=Cc, Hs=Hs, Ws=Ws, mode=_MODES[mode],
                  padding=_PADDINGS[padding], normalize=int(bool(normalize)), src_u8=int(src_u8), out_u8=int(out_dtype == torch.uint8),
                  out_rows=rows, src_shared=int(sb == 1), mask_shared=int(m is not None and m.shape[0] == 1))
        check(_lib.lib.ud_remap(desc, cur_stream()), "ud_remap")
    return (out, valid.view(torch.bool)) if return_mask else out


def undistort(src: torch.Tensor, src_camera, dst_camera=None, out_shape: Optional[Tuple[int, int]] = None, *, mode: str = "bilinear",
              padding: str = "zeros", src_mask: Optional[torch.Tensor] = None, normalize: bool = False, return_mask: bool = False,
              return_uv: bool = False):
    """Maps seen through src_camera resampled into the pixel grid of dst_camera (rectifying a fisheye image, bringing a prediction into
    another camera's pixels): for every pixel centre of the destination, the ray of dst_camera, projected through src_camera, sampled.

    src         [B,C,Hs,Ws] as remap takes it.
    src_camera  any of the six models, one per image, as gtpoints.prepare_camera takes it.
    dst_camera  the same; None: a Pinhole with the source's fx, fy, cx, cy (built on the device, nothing is read back).
    out_shape   (Ho, Wo) of the result; None: the source's.
    mode, padding, src_mask, normalize, return_mask: remap's.  return_uv=True appends project_camera's uv [B,2,Ho,Wo].

    It is exactly  rays = unproject_camera(None, dst_camera, image_shape=out_shape);
                   uv, inside, depth = project_camera(rays, src_camera, image_shape=(Hs, Ws));
                   remap(src, uv, coord_valid=inside & (depth > 0), ...)
    -- two launches and the sampler (unprojection launches twice more with an OPENCV or Fisheye624 destination), beside the two small
    element-wise operations of `inside & (depth > 0)`; the validity test stays on the device.  Nothing is fused.

    Values are RESAMPLED, not converted: a depth map moved between a model whose depth is z and Spherical, whose depth is the distance
    along the ray, keeps its numbers.  Converting them is the caller's business."""
    fn = "undistort"
    if not isinstance(src, torch.Tensor) or src.ndim != 4 or min(src.shape) == 0:
        raise ValueError(f"{fn}: src must be [B,C,Hs,Ws], non-empty, got {tuple(getattr(src, 'shape', ()))}")
    Hs, Ws = src.shape[-2:]
    if out_shape is None:
        out_shape = (Hs, Ws)
    Ho, Wo = _args.image_shape(fn, out_shape, "out_shape")
    B = max([src.shape[0], _args.n_cameras(src_camera)] + ([_args.n_cameras(dst_camera)] if dst_camera is not None else []))
    _args.batch_of(fn, "src", src.shape[0], B)
    _args.one_gpu(fn, src.device)
    cam_s = prepare_camera(src_camera, B, src.device)
    if dst_camera is None:
        rows = torch.zeros_like(cam_s.params)
        rows[:, :4] = cam_s.params[:, :4]
        cam_d = PreparedCamera(rows, (GT_PINHOLE,) * B)
    else:
        cam_d = prepare_camera(dst_camera, B, src.device)
    rays = unproject_camera(None, cam_d, image_shape=(Ho, Wo))
    uv, inside, depth = project_camera(rays, cam_s, image_shape=(Hs, Ws))
    res = remap(src, uv, mode=mode, padding=padding, src_mask=src_mask, coord_valid=inside & (depth > 0), normalize=normalize,
                return_mask=return_mask)
    res = res if return_mask else (res,)
    if return_uv:
        res = res + (uv,)
    return _args.tail(res)


def overlap_mask(projected: torch.Tensor) -> torch.Tensor:
    """The reference's Camera.mask_overlap_projection: projected fp32 [B,2,H,W], the image coordinates a projection gave the points of
    the pixel grid -> bool [B,1,H,W], False where the flow projected - grid, followed a tenth of its way, meets a flow shorter than 0.9 of
    its own (content folded over from another part of the image) and is at least a pixel long.  H, W >= 2.  One launch."""
    fn = "overlap_mask"
    _args.float_tensor(fn, "projected", projected)
    if projected.ndim != 4 or projected.shape[1] != 2 or projected.shape[0] == 0:
        raise ValueError(f"{fn}: projected must be [B,2,H,W], got {tuple(projected.shape)}")
    B, _, H, W = projected.shape
    if H < 2 or W < 2:
        raise ValueError(f"{fn}: H and W must be at least 2 (the sample grid divides by H - 1 and W - 1), got ({H}, {W})")
    _args.max_images(fn, B)
    _args.max_elems(fn, f"H={H} W={W}", H * W)
    _args.one_gpu(fn, projected.device)
    with torch.cuda.device(projected.device):
        uv = projected.float().contiguous()
        mask = torch.empty((B, 1, H, W), device=uv.device, dtype=torch.uint8)
        check(_lib.lib.ud_overlap_mask(mk(_lib.UdOverlapMask, uv=uv, mask=mask, B=B, H=H, W=W), cur_stream()), "ud_overlap_mask")
    return mask.view(torch.bool)


class _CallableModule(type(sys)):
    """`unidepth_amd.remap` names this module AND its function remap(): importing the module binds it over the package's lazy attribute
    of the same name, so the module itself answers a call as the function does (as reproject.py)."""

    def __call__(self, *args, **kw):
        return remap(*args, **kw)


sys.modules[__name__].__class__ = _CallableModule
