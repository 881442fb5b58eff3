"""Packed point clouds from infer() outputs, over ud_pointcloud_pack (include/unidepth_hip.h UdPointCloud, csrc/pointcloud.hip):

    pack_points, from_prediction, PointCloud     the valid pixels of a batch as packed xyz (+ rgb, + pixel index) rows, on the GPU
    get_pointcloud_from_rgbd, save_file_ply      unidepth/utils/visualization.py:57-104, 107-132 (same names, arguments and results)
    save_ply                                     binary little-endian PLY, one write

The compaction is ordered (images in batch order, pixels row-major: the order of numpy boolean indexing), bitwise reproducible and
stream-ordered; with `capacity` given it makes no host synchronisation.  Tensors must live on the GPU: there is no CPU path."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .ops import check, cur_stream, mk


@dataclass
class PointCloud:
    """xyz fp32 [capacity, 3]; rgb u8 or fp32 [capacity, 3] or None; index int32 [capacity] (y * W + x inside the image) or None;
    counts int64 [B] and offsets int64 [B + 1]: the TRUE number of valid pixels per image and its exclusive prefix, whatever the
    capacity (offsets[-1] > capacity means the rows from `capacity` on were dropped).  Rows from min(offsets[-1], capacity) on are
    unwritten memory."""
    xyz: torch.Tensor
    rgb: Optional[torch.Tensor]
    index: Optional[torch.Tensor]
    counts: torch.Tensor
    offsets: torch.Tensor

    def split(self) -> List["PointCloud"]:
        """One PointCloud of views per image (rows beyond the capacity are missing from the images they belong to).  SYNCHRONISES:
        the offsets are read back to the host."""
        off = [min(int(o), self.xyz.shape[0]) for o in self.offsets.cpu().tolist()]
        out = []
        for b in range(len(off) - 1):
            s = slice(off[b], off[b + 1])
            out.append(PointCloud(self.xyz[s], None if self.rgb is None else self.rgb[s], None if self.index is None else self.index[s],
                                  self.counts[b:b + 1], self.offsets[b:b + 2] - self.offsets[b]))
        return out


def _map(name, t, B, H, W, dtypes):
    """A [B,1,H,W] / [B,H,W] map -> contiguous [B,H,W] of its own dtype (bool viewed as uint8)."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise ValueError(f"pack_points: {name} must be a tensor of dtype {' or '.join(str(d) for d in dtypes)}")
    if tuple(t.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"pack_points: {name} must be [{B},1,{H},{W}] or [{B},{H},{W}], got {tuple(t.shape)}")
    t = t.reshape(B, H, W).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def pack_points(points: Optional[torch.Tensor] = None, *, depth: Optional[torch.Tensor] = None, intrinsics: Optional[torch.Tensor] = None,
                image: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, confidence: Optional[torch.Tensor] = None,
                min_confidence: Optional[float] = None, depth_range=None, edge_rtol: Optional[float] = None, flip_y: bool = False,
                capacity: Optional[int] = None, return_index: bool = False, workspace: Optional[torch.Tensor] = None) -> PointCloud:
    """The valid pixels of a batch as packed rows.  points fp32 [B,3,H,W] (copied bit-exactly) and / or depth fp32 [B,1,H,W] / [B,H,W];
    without points the rows are unprojected from depth with the pinhole `intrinsics` ([3,3], [1,3,3] or [B,3,3]; skew ignored):
    x = (u - cx) d / fx, y = (v - cy) d / fy, z = d in fp32.  image uint8 or fp32 [B,3,H,W] gives rgb rows of the same dtype.

    A pixel is kept when its mask (bool / uint8 [B,1,H,W] or [B,H,W]) is set, its coordinates (points) or depth are finite, and, with
    d = depth when given, else z:  confidence >= min_confidence;  depth_range[0] <= d <= depth_range[1];  |d - dn| <= edge_rtol min(d, dn)
    for each of its 4 neighbours dn inside the image (a flying-pixel filter; a non-finite neighbour drops the pixel).  flip_y negates y.

    capacity = int: outputs are [capacity, 3] and the call makes NO host synchronisation; counts / offsets still hold the true totals,
    so an overflow is detectable later.  capacity = None: counts first, reads the total back (one synchronisation) and allocates
    exactly that.  workspace: an optional contiguous, 8-byte aligned uint8 GPU tensor of at least ud_pointcloud_work_bytes(B, H, W)
    bytes to reuse."""
    if points is None and depth is None:
        raise ValueError("pack_points: points or depth is required")
    lead = points if points is not None else depth
    if not isinstance(lead, torch.Tensor) or lead.dtype != torch.float32:
        raise ValueError("pack_points: points / depth must be fp32 tensors")
    if points is not None:
        if points.ndim != 4 or points.shape[1] != 3:
            raise ValueError(f"pack_points: points must be [B,3,H,W], got {tuple(points.shape)}")
        B, _, H, W = points.shape
    else:
        if depth.ndim not in (3, 4) or (depth.ndim == 4 and depth.shape[1] != 1):
            raise ValueError(f"pack_points: depth must be [B,1,H,W] or [B,H,W], got {tuple(depth.shape)}")
        B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    if B <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"pack_points: empty input (B={B}, H={H}, W={W})")
    tensors = {}
    if points is not None:
        tensors["points"] = points.contiguous()
    if depth is not None:
        tensors["depth"] = _map("depth", depth, B, H, W, (torch.float32,))
    nK = 0
    if points is None:
        if intrinsics is None:
            raise ValueError("pack_points: depth without points needs intrinsics")
        if not isinstance(intrinsics, torch.Tensor) or intrinsics.dtype != torch.float32 or tuple(intrinsics.shape) not in ((3, 3), (1, 3, 3), (B, 3, 3)):
            raise ValueError(f"pack_points: intrinsics must be fp32 [3,3], [1,3,3] or [{B},3,3]")
        tensors["K"] = intrinsics.reshape(-1, 3, 3).contiguous()
        nK = tensors["K"].shape[0]
    if image is not None:
        if not isinstance(image, torch.Tensor) or image.dtype not in (torch.uint8, torch.float32) or tuple(image.shape) != (B, 3, H, W):
            raise ValueError(f"pack_points: image must be uint8 or fp32 [{B},3,{H},{W}]")
        tensors["image" if image.dtype == torch.uint8 else "image_f32"] = image.contiguous()
    if mask is not None:
        tensors["mask"] = _map("mask", mask, B, H, W, (torch.bool, torch.uint8))
    flags = _lib.UD_PC_FLIP_Y if flip_y else 0
    min_conf = dmin = dmax = rtol = 0.0
    if min_confidence is not None:
        if confidence is None:
            raise ValueError("pack_points: min_confidence without confidence")
        tensors["confidence"] = _map("confidence", confidence, B, H, W, (torch.float32,))
        flags |= _lib.UD_PC_MINCONF
        min_conf = float(min_confidence)
    if depth_range is not None:
        try:
            dmin, dmax = (float(v) for v in depth_range)
        except (TypeError, ValueError):
            raise ValueError("pack_points: depth_range must be a (min, max) pair") from None
        flags |= _lib.UD_PC_RANGE
    if edge_rtol is not None:
        flags |= _lib.UD_PC_EDGE
        rtol = float(edge_rtol)
    nbytes = int(_lib.lib.ud_pointcloud_work_bytes(B, H, W))
    if nbytes < 0 or (return_index and B * H * W > 2 ** 31 - 1):
        raise ValueError(f"pack_points: unsupported sizes B={B} H={H} W={W}")

    def run(cap, xyz, rgb, index, **work):
        d = mk(_lib.UdPointCloud, xyz=xyz, rgb=rgb, index=index, capacity=cap, B=B, H=H, W=W, nK=nK, flags=flags, min_conf=min_conf, dmin=dmin,
               dmax=dmax, edge_rtol=rtol, **tensors, **work)
        check(_lib.lib.ud_pointcloud_pack(d, cur_stream()), "ud_pointcloud_pack")

    return _packed("pack_points", lead.device, B, nbytes, run, capacity, workspace, None if image is None else image.dtype, return_index,
                   inputs=tensors)


def _packed(fn, dev, B, nbytes, run, capacity, workspace, rgb_dtype, want_index, inputs=None) -> PointCloud:
    """The tail every packer over csrc/compact.h shares (pack_points, tsdf.tsdf_points): the checks of `capacity` and `workspace` (nbytes:
    what the packer's *_work_bytes() asks for) in fn's own sentences, counts / offsets, and run(cap, xyz, rgb, index, **work) -- the
    packer's one C call, `work` being the descriptor's counts, offsets, work and work_bytes -- once with the given capacity (no host
    synchronisation), or count-only, one read-back, then exactly the total.  rgb_dtype None: no rgb rows; inputs: named tensors that must
    live on dev."""
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0):
        raise ValueError(f"{fn}: capacity must be a non-negative int or None")
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev
                                  or not workspace.is_contiguous() or workspace.numel() < nbytes or workspace.data_ptr() % 8):
        raise ValueError(f"{fn}: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least {nbytes} bytes on {dev}")
    for name, t in (inputs or {}).items():
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{fn}: {name} must live on the GPU of the first input ({dev}); there is no CPU path")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        counts = torch.empty(B, device=dev, dtype=torch.int64)
        offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
        work = dict(counts=counts, offsets=offsets, work=workspace, work_bytes=workspace.numel())
        counted = capacity is None
        if counted:
            run(0, None, None, None, **work)               # count only
            capacity = int(offsets[B].item())              # the one synchronisation
        xyz = torch.empty(capacity, 3, device=dev, dtype=torch.float32)
        rgb = torch.empty(capacity, 3, device=dev, dtype=rgb_dtype) if rgb_dtype is not None else None
        index = torch.empty(capacity, device=dev, dtype=torch.int32) if want_index else None
        if capacity > 0:
            run(capacity, xyz, rgb, index, **work)
        elif not counted:
            run(0, None, None, None, **work)
    return PointCloud(xyz, rgb, index, counts, offsets)


def from_prediction(out, image: Optional[torch.Tensor] = None, **filters) -> PointCloud:
    """pack_points on an infer() dict of UniDepthV1 / V2: its `points` are the rows, its `depth` (when present) the depth source of the
    range and edge filters, its `confidence` (when present) the map behind min_confidence.  Usable as
    InferPipeline.submit(..., post=lambda o: clouds.append(from_prediction(o, capacity=N))): it runs on the call's stream."""
    if "points" not in out:
        raise ValueError("from_prediction: the prediction has no 'points'")
    return pack_points(out["points"], depth=out.get("depth"), confidence=out.get("confidence"), image=image, **filters)


def get_pointcloud_from_rgbd(image: np.ndarray, depth: np.ndarray, mask: np.ndarray, intrinsic_matrix: np.ndarray,
                             extrinsic_matrix: Optional[np.ndarray] = None) -> np.ndarray:
    """The reference's helper (utils/visualization.py:57-104): image [H,W,C], depth and mask [H,W] (squeezed), a 3x3 pinhole matrix ->
    one float64 [N, 3 + C] array of (x, y, z, colours) of the masked pixels in row-major order, +y up.  The unprojection and the
    compaction run on the GPU (depth mode with UD_PC_FLIP_Y) in fp32, where the reference computes x and y in float64: they agree to
    three fp32 roundings; z and the colours are the inputs.  Pixels with a non-finite depth are dropped (the reference keeps them).
    The reference's extrinsics branch is commented out: None is accepted, a matrix raises."""
    if extrinsic_matrix is not None:
        raise NotImplementedError("get_pointcloud_from_rgbd: extrinsic_matrix is not supported (the reference ignores it)")
    depth = np.array(depth).squeeze()
    mask = np.array(mask).squeeze()
    image = np.asarray(image)
    if depth.ndim != 2 or mask.shape != depth.shape or image.shape[:2] != depth.shape:
        raise ValueError(f"get_pointcloud_from_rgbd: image {image.shape}, depth {depth.shape} and mask {mask.shape} do not match")
    dev = torch.device("cuda", torch.cuda.current_device())
    d = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))[None].to(dev)
    m = torch.from_numpy(np.ascontiguousarray(mask != False))[None].to(dev)              # noqa: E712 (the reference's own test)
    K = torch.from_numpy(np.ascontiguousarray(np.asarray(intrinsic_matrix), dtype=np.float32)).to(dev)
    pc = pack_points(depth=d, intrinsics=K, mask=m, flip_y=True, return_index=True)
    idx = pc.index.cpu().numpy().astype(np.int64)
    colours = image.reshape(depth.size, -1)[idx]
    return np.concatenate([pc.xyz.cpu().numpy().astype(np.float64), colours], axis=-1)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _rgb_u8(rgb: np.ndarray) -> np.ndarray:
    if rgb.dtype == np.uint8:
        return rgb
    if rgb.size and rgb.max() < 1.001:                    # the reference's rule: colours in [0, 1] are scaled to [0, 255]
        rgb = rgb * 255.0
    return rgb.astype(np.uint8)


def save_ply(path, xyz, rgb=None) -> None:
    """Binary little-endian PLY of xyz [N,3] (stored as float32) and optional rgb [N,3] (uint8 as is; floats by the reference's rule:
    scaled by 255 when their maximum is below 1.001).  Tensors or arrays; one write of a structured array."""
    xyz = _host(xyz)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"save_ply: xyz must be [N,3], got {xyz.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if rgb is not None:
        rgb = _rgb_u8(_host(rgb))
        if rgb.shape != xyz.shape:
            raise ValueError(f"save_ply: rgb must be [N,3] like xyz, got {rgb.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rows = np.empty(xyz.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate("xyz"):
        rows[name] = xyz[:, k]
    if rgb is not None:
        for k, name in enumerate(("red", "green", "blue")):
            rows[name] = rgb[:, k]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {xyz.shape[0]}"]
    header += [f"property {'float' if t == '<f4' else 'uchar'} {name}" for name, t in fields]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        rows.tofile(f)


def save_file_ply(xyz, rgb, pc_file) -> None:
    """The reference's ASCII writer (utils/visualization.py:107-132): its header, its `rgb.max() < 1.001` rule, one
    "%10.6f %10.6f %10.6f %d %d %d" row per point."""
    xyz, rgb = _host(xyz), _host(rgb)
    if rgb.max() < 1.001:
        rgb = rgb * 255.0
    rgb = rgb.astype(np.uint8)
    lines = ["ply\nformat ascii 1.0\n", f"element vertex {xyz.shape[0]}\n", "property float x\n", "property float y\n", "property float z\n",
             "property uchar red\n", "property uchar green\n", "property uchar blue\n", "end_header\n"]
    lines += ["{:10.6f} {:10.6f} {:10.6f} {:d} {:d} {:d}\n".format(xyz[i, 0], xyz[i, 1], xyz[i, 2], rgb[i, 0], rgb[i, 1], rgb[i, 2])
              for i in range(xyz.shape[0])]
    with open(pc_file, "w") as f:
        f.writelines(lines)
