"""Outputs matched to the ground truth, over ud_match_gt (include/unidepth_hip.h UdMatchGt, csrc/matchgt.hip):

    match_gt, match_intrinsics      unidepth/utils/misc.py:596-690 (same names, arguments and result shapes)

The reference loops over the images in Python (slice the padded window, F.interpolate, F.pad, torch.cat), once per map; here a batch
whose images carry different paddings is ONE stream-ordered launch for up to four maps and the intrinsics together
(UniDepthV2.forward_test issues exactly one).  Paddings are (left, right, top, bottom) per image, read and validated on the host."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import check
from .ops import cur_stream

__all__ = ["match_gt", "match_intrinsics"]


def host_paddings(padding, B: int, H: int, W: int, name: str) -> Optional[list]:
    """None, a sequence or a tensor of (l, r, t, b) per image -> a list of B int 4-tuples (None stays None); ValueError unless every
    entry is non-negative and leaves a window of at least 1 x 1 of the H x W map."""
    if padding is None:
        return None
    if isinstance(padding, torch.Tensor):
        padding = padding.detach().cpu().tolist()
    rows = [tuple(p.tolist() if isinstance(p, torch.Tensor) else p) for p in padding]
    if len(rows) != B or any(len(r) != 4 for r in rows):
        raise ValueError(f"{name}: one (left, right, top, bottom) per image expected, {B} images, got {rows}")
    out = []
    for i, r in enumerate(rows):
        if any(int(v) != v for v in r):
            raise ValueError(f"{name}[{i}]: integer paddings expected, got {r}")
        l, rr, t, b = (int(v) for v in r)
        if min(l, rr, t, b) < 0:
            raise ValueError(f"{name}[{i}]: negative padding {r}")
        if H - t - b < 1 or W - l - rr < 1:
            raise ValueError(f"{name}[{i}]: paddings {r} leave an empty window of a {H} x {W} map")
        out.append((l, rr, t, b))
    return out


def upload_paddings(p1: Optional[list], p2: Optional[list], device) -> tuple:
    """Both padding lists as ONE small int32 device tensor -> (pads1 or None, pads2 or None) views of it."""
    rows = (p1 or []) + (p2 or [])
    if not rows:
        return None, None
    t = torch.tensor(rows, dtype=torch.int32).to(device, non_blocking=True)
    n1 = len(p1 or [])
    return (t[:n1] if p1 else None), (t[n1:] if p2 else None)


def launch(planes: Sequence[dict], B: int, h1: int, w1: int, H2: int, W2: int, pads1, pads2, K_in=None, K_out=None):
    """One ud_match_gt on the current stream.  planes: dicts of src, dst, C, src_batch_stride (floats) and optionally mul; tensors or raw
    device addresses.  pads1 / pads2: int32 device tensors [B,4] or None."""
    d = _lib.UdMatchGt()
    assert len(planes) <= _lib.UD_MATCH_MAX_PLANES
    for i, p in enumerate(planes):
        for k, v in p.items():
            setattr(d.planes[i], k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    d.n_planes, d.B, d.h1, d.w1, d.H2, d.W2 = len(planes), B, h1, w1, H2, W2
    for k, v in (("pads1", pads1), ("pads2", pads2), ("K_in", K_in), ("K_out", K_out)):
        setattr(d, k, None if v is None else v.data_ptr())
    check(_lib.lib.ud_match_gt(C.byref(d), cur_stream()), "ud_match_gt")


def _geometry(tensor1, tensor2, padding1, padding2, who):
    for name, t in (("tensor1", tensor1), ("tensor2", tensor2)):
        if not isinstance(t, torch.Tensor) or t.ndim != 4:
            raise ValueError(f"{who}: {name} must be [B,C,H,W], got {tuple(getattr(t, 'shape', ()))}")
    B, _, h1, w1 = tensor1.shape
    H2, W2 = tensor2.shape[-2:]
    if B < 1 or min(h1, w1, H2, W2) < 1:
        raise ValueError(f"{who}: empty tensor ({tuple(tensor1.shape)} -> {tuple(tensor2.shape)})")
    if tensor2.shape[0] != B:
        raise ValueError(f"{who}: batch sizes differ (tensor1 {B}, tensor2 {tensor2.shape[0]})")
    p1 = host_paddings(padding1, B, h1, w1, f"{who}: padding1")
    p2 = host_paddings(padding2, B, H2, W2, f"{who}: padding2")
    return B, h1, w1, H2, W2, p1, p2


def match_gt(tensor1: torch.Tensor, tensor2: torch.Tensor, padding1, padding2, mode: str = "bilinear") -> torch.Tensor:
    """Every image of tensor1 [B,C,h1,w1] without its padding1, bilinearly resampled (align_corners=False) to tensor2's size without
    padding2 and zero-padded by padding2 -> [B,C,H2,W2] (utils/misc.py:596-642).  tensor2 [B,*,H2,W2] gives the size only.  paddings: None,
    a sequence or a tensor of (left, right, top, bottom) per image.  fp32 arithmetic (other float dtypes are converted, the result is cast
    back to tensor1's dtype); one ud_match_gt launch, bitwise reproducible."""
    if mode != "bilinear":
        raise ValueError(f"match_gt: mode {mode!r}: only 'bilinear' is implemented")
    B, h1, w1, H2, W2, p1, p2 = _geometry(tensor1, tensor2, padding1, padding2, "match_gt")
    if not tensor1.is_cuda:
        raise RuntimeError("match_gt: GPU tensors expected (the HIP kernels are the only implementation)")
    Cn = tensor1.shape[1]
    with torch.cuda.device(tensor1.device):
        src = tensor1.detach().float().contiguous()
        out = torch.empty(B, Cn, H2, W2, dtype=torch.float32, device=tensor1.device)
        d1, d2 = upload_paddings(p1, p2, tensor1.device)
        launch([dict(src=src, dst=out, C=Cn, src_batch_stride=Cn * h1 * w1)], B, h1, w1, H2, W2, d1, d2)
    return out.to(tensor1.dtype)


def match_intrinsics(K1: torch.Tensor, tensor1: torch.Tensor, tensor2: torch.Tensor, padding1, padding2) -> torch.Tensor:
    """The intrinsics K1 [B,3,3] of tensor1 after the crop / resize / pad that match_gt applies (utils/misc.py:645-690): focal lengths
    scaled by the window ratio, principal point moved by the paddings.  The same ud_match_gt call with no planes."""
    if not isinstance(K1, torch.Tensor) or K1.ndim != 3 or tuple(K1.shape[1:]) != (3, 3):
        raise ValueError(f"match_intrinsics: K1 must be [B,3,3], got {tuple(getattr(K1, 'shape', ()))}")
    B, h1, w1, H2, W2, p1, p2 = _geometry(tensor1, tensor2, padding1, padding2, "match_intrinsics")
    if K1.shape[0] != B:
        raise ValueError(f"match_intrinsics: batch sizes differ (K1 {K1.shape[0]}, tensor1 {B})")
    if not K1.is_cuda:
        raise RuntimeError("match_intrinsics: GPU tensors expected (the HIP kernels are the only implementation)")
    with torch.cuda.device(K1.device):
        Kin = K1.detach().float().contiguous()
        Kout = torch.empty_like(Kin)
        d1, d2 = upload_paddings(p1, p2, K1.device)
        launch([], B, h1, w1, H2, W2, d1, d2, Kin, Kout)
    return Kout.to(K1.dtype)
