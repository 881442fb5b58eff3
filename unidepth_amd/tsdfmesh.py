"""The surface of a TsdfVolume as an indexed triangle mesh, the last stage after tsdf_integrate: vertices and faces a viewer shades.

    TriangleMesh                        packed vertices (+ rgb, + normals) and int32 faces of a batch of volumes, with counts and offsets
    tsdf_mesh(volume, ...)              one ud_tsdf_mesh call (csrc/tsdf_mesh.hip): two ordered compactions, cells -> vertices, slots -> quads
    tsdf_mesh_composition(volume, ...)  the same definition in vectorised torch, on any device
    save_mesh_ply(path, ...)            binary little-endian PLY with a face list

Naive surface nets: no case table.  A CELL is the cube between a voxel and its seven +x / +y / +z neighbours; it is live when all eight
weights are >= min_weight, no distance is a NaN and the corners differ in sign.  A live cell carries one vertex, the mean of the crossing
points of its edges (tsdf_points' points, the same bits); an edge with a sign change whose four surrounding cells are live carries one
quad between their vertices, wound so that its normal points to the positive (free-space) side, and split into two triangles.  The order
is fixed (volumes, then cells / edges in voxel order) and every bit reproducible.  The HIP kernels are the only implementation of
tsdf_mesh: CPU tensors raise."""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _args, _lib
from .ops import check, cur_stream, mk
from .pointcloud import _host, _rgb_u8
from .tsdf import TsdfVolume, _check_volume


@dataclass
class TriangleMesh:
    """vertices fp32 [vert_capacity, 3]; faces int32 [face_capacity, 3], vertex rows LOCAL to the volume (row - vert_offsets[b]); rgb u8
    or fp32 [vert_capacity, 3] or None; normals fp32 [vert_capacity, 3] or None; vert_counts / face_counts int64 [B] and vert_offsets /
    face_offsets int64 [B + 1]: the TRUE numbers of vertices and triangles per volume and their exclusive prefixes, whatever the
    capacities (an offset above the capacity means the rows from the capacity on were dropped).  Rows from min(total, capacity) on are
    unwritten memory."""
    vertices: torch.Tensor
    faces: torch.Tensor
    rgb: Optional[torch.Tensor]
    normals: Optional[torch.Tensor]
    vert_counts: torch.Tensor
    vert_offsets: torch.Tensor
    face_counts: torch.Tensor
    face_offsets: torch.Tensor

    def split(self) -> List["TriangleMesh"]:
        """One self-contained TriangleMesh of views per volume (rows beyond a capacity are missing from the volumes they belong to).
        SYNCHRONISES: the offsets are read back to the host."""
        vo = [min(int(o), self.vertices.shape[0]) for o in self.vert_offsets.cpu().tolist()]
        fo = [min(int(o), self.faces.shape[0]) for o in self.face_offsets.cpu().tolist()]
        out = []
        for b in range(len(vo) - 1):
            v, f = slice(vo[b], vo[b + 1]), slice(fo[b], fo[b + 1])
            out.append(TriangleMesh(self.vertices[v], self.faces[f], None if self.rgb is None else self.rgb[v],
                                    None if self.normals is None else self.normals[v], self.vert_counts[b:b + 1],
                                    self.vert_offsets[b:b + 2] - self.vert_offsets[b], self.face_counts[b:b + 1],
                                    self.face_offsets[b:b + 2] - self.face_offsets[b]))
        return out


def _min_weight(fn, min_weight):
    """a Python number as (the value of its fp32 rounding, that rounding's bit pattern); not a NaN -- tsdf_points' sentences"""
    try:
        bits = _args.f32_bits(float(min_weight))
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: min_weight must be a number in fp32's range") from None
    if isinstance(min_weight, bool) or math.isnan(float(min_weight)):
        raise ValueError(f"{fn}: min_weight must be a number, got {min_weight}")
    return struct.unpack("<f", struct.pack("<i", bits))[0], bits


def _rgb_dtype(fn, rgb_dtype):
    if rgb_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{fn}: rgb_dtype must be torch.uint8 or torch.float32, got {rgb_dtype}")


def tsdf_mesh(volume: TsdfVolume, *, min_weight: float = 1.0, vert_capacity: Optional[int] = None, face_capacity: Optional[int] = None,
              rgb_dtype: torch.dtype = torch.uint8, return_normals: bool = False, workspace: Optional[torch.Tensor] = None) -> TriangleMesh:
    """The surface of a TsdfVolume as a packed TriangleMesh (naive surface nets; the definition is written out at UdTsdfMesh in
    include/unidepth_hip.h and in csrc/tsdf_mesh_point.h).

    One vertex per live cell -- the cube of voxel (ix, iy, iz) and its +x / +y / +z neighbours, all eight weights >= min_weight, no
    distance a NaN, not all of one sign -- at the mean of tsdf_points' crossing points on the cell's edges; with volume.color the mean of
    their colours as rgb_dtype (torch.uint8, rounded half to even and clamped, or torch.float32); with return_normals the normalised
    gradient of the cell's corners, pointing to the positive side.  One quad, as two triangles, per crossing edge whose four cells are
    live; faces index the vertices of their own volume from 0, so each volume's slice is a self-contained mesh.  A live cell without a
    complete quad leaves an unreferenced vertex.

    The order is fixed (volumes in batch order, then cells and edges in voxel order, x fastest) and every bit reproducible.
    vert_capacity and face_capacity (in triangles) both ints: the outputs have those sizes and the call makes NO host synchronisation
    (it captures into a graph); the counts and offsets still hold the true totals, so an overflow is detectable later; a quad is written
    only when both its triangles fit.  Both None: counts first, reads both totals back (one synchronisation) and allocates exactly
    those.  Exactly one of them: ValueError.  workspace: an optional uint8 GPU tensor of at least ud_tsdf_mesh_work_bytes(B, Nx, Ny,
    Nz) bytes to reuse.
    -> TriangleMesh; save_mesh_ply(path, m.vertices, m.faces, m.rgb, m.normals) takes a single volume's mesh as it is."""
    fn = "tsdf_mesh"
    if not isinstance(volume, TsdfVolume):
        raise ValueError(f"{fn}: volume must be a TsdfVolume, got {type(volume).__name__}")
    _, mw_bits = _min_weight(fn, min_weight)
    _rgb_dtype(fn, rgb_dtype)
    for name, cap in (("vert_capacity", vert_capacity), ("face_capacity", face_capacity)):
        if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int) or cap < 0):
            raise ValueError(f"{fn}: {name} must be a non-negative int or None")
    if (vert_capacity is None) != (face_capacity is None):
        raise ValueError(f"{fn}: vert_capacity and face_capacity go together (both ints, or both None)")
    B, Nz, Ny, Nx, _, vs_bits = _check_volume(fn, volume)
    nbytes = int(_lib.lib.ud_tsdf_mesh_work_bytes(B, Nx, Ny, Nz))
    if nbytes < 0:
        raise ValueError(f"{fn}: unsupported sizes B={B} grid={Nz}x{Ny}x{Nx} (3 * Nx * Ny * Nz must stay below 2^31 - 256)")
    dev = volume.tsdf.device
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev
                                  or not workspace.is_contiguous() or workspace.numel() < nbytes or workspace.data_ptr() % 8):
        raise ValueError(f"{fn}: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least {nbytes} bytes on {dev}")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        totals = torch.empty(4 * B + 2, device=dev, dtype=torch.int64)             # one allocation, so that one read-back brings both totals
        vert_counts, vert_offsets, face_counts, face_offsets = totals.split((B, B + 1, B, B + 1))

        def run(vcap, fcap, vertices, rgb, normals, faces):
            d = mk(_lib.UdTsdfMesh, tsdf=volume.tsdf, weight=volume.weight, color=volume.color, origin=volume.origin, vertices=vertices, rgb=rgb,
                   normals=normals, faces=faces, vert_counts=vert_counts, vert_offsets=vert_offsets, face_counts=face_counts,
                   face_offsets=face_offsets, work=workspace, work_bytes=workspace.numel(), vert_capacity=vcap, face_capacity=fcap, B=B, Nx=Nx,
                   Ny=Ny, Nz=Nz, n_origin=volume.origin.shape[0], rgb_f32=int(rgb_dtype == torch.float32), voxel_size_bits=vs_bits,
                   min_weight_bits=mw_bits)
            check(_lib.lib.ud_tsdf_mesh(d, cur_stream()), "ud_tsdf_mesh")

        counted = vert_capacity is None
        if counted:
            run(0, 0, None, None, None, None)                # count only
            host = totals.cpu()                              # the one synchronisation
            vert_capacity, face_capacity = int(host[2 * B]), int(host[4 * B + 1])
        vertices = torch.empty(vert_capacity, 3, device=dev, dtype=torch.float32)
        faces = torch.empty(face_capacity, 3, device=dev, dtype=torch.int32)
        rgb = torch.empty(vert_capacity, 3, device=dev, dtype=rgb_dtype) if volume.color is not None else None
        normals = torch.empty(vert_capacity, 3, device=dev, dtype=torch.float32) if return_normals else None
        if vert_capacity > 0 or face_capacity > 0:
            run(vert_capacity, face_capacity, vertices if vert_capacity > 0 else None, rgb if vert_capacity > 0 else None,
                normals if vert_capacity > 0 else None, faces if face_capacity > 0 else None)
        elif not counted:
            run(0, 0, None, None, None, None)
    return TriangleMesh(vertices, faces, rgb, normals, vert_counts, vert_offsets, face_counts, face_offsets)


# ---- the same definition in torch ------------------------------------------------------------------------------------------------------

def _compose_volume(fn, volume):
    """a TsdfVolume of fp32 tensors on ONE device, any device -> (B, Nz, Ny, Nx, voxel size)"""
    if not isinstance(volume, TsdfVolume):
        raise ValueError(f"{fn}: volume must be a TsdfVolume, got {type(volume).__name__}")
    t = volume.tsdf
    ok = lambda x: isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device == t.device  # noqa: E731
    if not isinstance(t, torch.Tensor) or t.ndim != 4 or min(t.shape) == 0 or not ok(t):
        raise ValueError(f"{fn}: volume.tsdf must be an fp32 tensor [B,Nz,Ny,Nx], non-empty")
    B, Nz, Ny, Nx = t.shape
    if not ok(volume.weight) or volume.weight.shape != t.shape:
        raise ValueError(f"{fn}: volume.weight must be an fp32 tensor shaped like volume.tsdf {tuple(t.shape)}, on its device")
    if volume.color is not None and (not ok(volume.color) or tuple(volume.color.shape) != (B, 3, Nz, Ny, Nx)):
        raise ValueError(f"{fn}: volume.color must be None or an fp32 tensor [{B},3,{Nz},{Ny},{Nx}], on volume.tsdf's device")
    if not ok(volume.origin) or tuple(volume.origin.shape) not in ((1, 3), (B, 3)):
        raise ValueError(f"{fn}: volume.origin must be an fp32 tensor [1,3] or [{B},3], on volume.tsdf's device")
    try:
        bits = _args.f32_bits(float(volume.voxel_size))
    except (TypeError, ValueError, OverflowError, struct.error):
        raise ValueError(f"{fn}: volume.voxel_size must be a number in fp32's range") from None
    vs = struct.unpack("<f", struct.pack("<i", bits))[0]
    if isinstance(volume.voxel_size, bool) or not (vs > 0.0 and math.isfinite(vs)):
        raise ValueError(f"{fn}: volume.voxel_size must be finite and positive, got {volume.voxel_size}")
    if 3 * Nx * Ny * Nz >= 2 ** 31 - 256:
        raise ValueError(f"{fn}: unsupported sizes B={B} grid={Nz}x{Ny}x{Nx} (3 * Nx * Ny * Nz must stay below 2^31 - 256)")
    return B, Nz, Ny, Nx, vs


def _to_u8(x):
    return torch.where(torch.isnan(x), torch.zeros_like(x), torch.round(x).clamp(0, 255)).to(torch.uint8)


def tsdf_mesh_composition(volume: TsdfVolume, *, min_weight: float = 1.0, rgb_dtype: torch.dtype = torch.uint8,
                          return_normals: bool = False) -> TriangleMesh:
    """tsdf_mesh's definition spelled in vectorised torch, on the volume's device (CPU tensors are accepted): arguments and the result
    as there, the capacities being the totals.  The eight corners of every cell as shifted views; twelve masked accumulation steps, one
    per edge in edge order, for the vertex (and colour) sums; nonzero for the live cells; a cumulative sum over the cell mask as the map
    from a cell to its vertex row; per axis the edge's own test and the four shifted cell masks, nonzero over (voxel, axis) for the
    quads in slot order, and gathers through the row map for the indices.  Some hundred launches, each a pass over the volume.  This is
    the second oracle of the fused kernels' tests, after the numpy restatement, and the counterpart of their benchmark."""
    fn = "tsdf_mesh_composition"
    B, Nz, Ny, Nx, vs = _compose_volume(fn, volume)
    mw, _ = _min_weight(fn, min_weight)
    _rgb_dtype(fn, rgb_dtype)
    t, w, col, o = volume.tsdf, volume.weight, volume.color, volume.origin
    dev = t.device
    i64 = dict(device=dev, dtype=torch.int64)
    cz, cy, cx = Nz - 1, Ny - 1, Nx - 1
    zeros = torch.zeros(B, **i64)
    if min(cz, cy, cx) == 0:                                                       # no cells: an empty mesh
        return TriangleMesh(torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev, dtype=torch.int32),
                            None if col is None else torch.empty(0, 3, device=dev, dtype=rgb_dtype),
                            torch.empty(0, 3, device=dev) if return_normals else None, zeros, torch.zeros(B + 1, **i64), zeros.clone(),
                            torch.zeros(B + 1, **i64))

    def corner(a, c):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        return a[..., dz:dz + cz, dy:dy + cy, dx:dx + cx]

    d = [corner(t, c) for c in range(8)]
    ok, any_neg, any_pos = None, None, None
    for c in range(8):
        good = (corner(w, c) >= mw) & ~torch.isnan(d[c])
        neg = d[c] < 0
        ok = good if ok is None else ok & good
        any_neg = neg if any_neg is None else any_neg | neg
        any_pos = ~neg if any_pos is None else any_pos | ~neg
    live = ok & any_neg & any_pos                                                  # [B,cz,cy,cx]
    # the voxel centres per axis, [nO, N]: origin + (index + 0.5) * voxel_size
    centre = [o[:, k:k + 1] + (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * vs for k, n in enumerate((Nx, Ny, Nz))]
    shape1 = ((1, 1, -1), (1, -1, 1), (-1, 1, 1))
    cells = (cx, cy, cz)
    acc = [torch.zeros_like(d[0]) for _ in range(3)]
    cacc = [torch.zeros_like(d[0]) for _ in range(3)] if col is not None else None
    count = torch.zeros(live.shape, device=dev, dtype=torch.int32)
    for e in range(12):
        axis, k = e >> 2, e & 3
        o0, o1 = [x for x in range(3) if x != axis]
        off = [0, 0, 0]
        off[o0], off[o1] = k & 1, (k >> 1) & 1
        lo = off[0] + 2 * off[1] + 4 * off[2]
        hi = lo + (1 << axis)
        d0, d1 = d[lo], d[hi]
        m = live & ((d0 < 0) != (d1 < 0))
        tt = d0 / (d0 - d1)
        first = count == 0
        for c in range(3):
            p = centre[c][:, off[c]:off[c] + cells[c]].reshape((-1,) + tuple(cells[c] if s == -1 else 1 for s in shape1[c]))
            if c == axis:
                p = p + tt * vs
            acc[c] = torch.where(m, torch.where(first, p.expand_as(acc[c]), acc[c] + p), acc[c])
        if col is not None:
            for c in range(3):
                c0, c1 = corner(col[:, c], lo), corner(col[:, c], hi)
                v = c0 + tt * (c1 - c0)
                cacc[c] = torch.where(m, torch.where(first, v, cacc[c] + v), cacc[c])
        count = count + m.to(torch.int32)
    cnt = count[live].float()
    vertices = torch.stack([a[live] / cnt for a in acc], dim=1)
    rgb = None
    if col is not None:
        rgb = torch.stack([a[live] / cnt for a in cacc], dim=1)
        if rgb_dtype == torch.uint8:
            rgb = _to_u8(rgb)
    normals = None
    if return_normals:
        dl = [x[live] for x in d]
        g0 = (((dl[1] - dl[0]) + (dl[3] - dl[2])) + (dl[5] - dl[4])) + (dl[7] - dl[6])
        g1 = (((dl[2] - dl[0]) + (dl[3] - dl[1])) + (dl[6] - dl[4])) + (dl[7] - dl[5])
        g2 = (((dl[4] - dl[0]) + (dl[5] - dl[1])) + (dl[6] - dl[2])) + (dl[7] - dl[3])
        # sqrtf, correctly rounded: the root in fp64 rounded to fp32 (torch's vectorised fp32 root on the CPU is an ulp off now and then)
        length = torch.sqrt(((g0 * g0 + g1 * g1) + g2 * g2).double()).float()
        good = (length > 0) & torch.isfinite(length)
        normals = torch.stack([torch.where(good, g / length, torch.zeros_like(g)) for g in (g0, g1, g2)], dim=1)
    # the cell mask over the whole voxel grid (border voxels have no cell) and the map from a cell to its vertex row inside its volume
    full = torch.zeros(t.shape, device=dev, dtype=torch.bool)
    full[:, :cz, :cy, :cx] = live
    rows = (torch.cumsum(full.reshape(B, -1).to(torch.int64), dim=1) - 1).to(torch.int32)
    vert_counts = full.reshape(B, -1).sum(dim=1)

    def below(mask, dim):
        """mask moved up by one along dim: out[c] = mask[c - e_dim], false where c has no such neighbour"""
        out = torch.zeros_like(mask)
        n = mask.shape[dim]
        out.narrow(dim, 1, n - 1).copy_(mask.narrow(dim, 0, n - 1))
        return out

    dims = (3, 2, 1)                                                               # the tensor dimension of the axes x, y, z
    quads = torch.zeros(t.shape + (3,), device=dev, dtype=torch.bool)
    wok = (w >= mw) & ~torch.isnan(t)
    for axis in range(3):
        dim, n = dims[axis], t.shape[dims[axis]]
        a, b = t.narrow(dim, 0, n - 1), t.narrow(dim, 1, n - 1)
        edge = torch.zeros_like(full)
        edge.narrow(dim, 0, n - 1).copy_(wok.narrow(dim, 0, n - 1) & wok.narrow(dim, 1, n - 1) & ((a < 0) != (b < 0)))
        du, dv = dims[(axis + 1) % 3], dims[(axis + 2) % 3]
        quads[..., axis] = edge & full & below(full, du) & below(full, dv) & below(below(full, du), dv)
    ib, iz, iy, ix, ia = quads.nonzero().unbind(1)                                 # volumes, then voxels x fastest, then axes: slot order
    lin = (iz * Ny + iy) * Nx + ix
    stride = torch.tensor([1, Nx, Nx * Ny], **i64)
    eu, ev = stride[(ia + 1) % 3], stride[(ia + 2) % 3]
    neg = t[ib, iz, iy, ix] < 0
    q0, q1, q2, q3 = lin - eu - ev, lin - ev, lin, lin - eu
    r = [rows[ib, q] for q in (q0, torch.where(neg, q1, q3), q2, torch.where(neg, q3, q1))]
    faces = torch.stack([torch.stack([r[0], r[1], r[2]], dim=1), torch.stack([r[0], r[2], r[3]], dim=1)], dim=1).reshape(-1, 3)
    face_counts = 2 * quads.reshape(B, -1).sum(dim=1)
    offsets = lambda c: torch.cat([torch.zeros(1, **i64), torch.cumsum(c, dim=0)])  # noqa: E731
    return TriangleMesh(vertices, faces, rgb, normals, vert_counts, offsets(vert_counts), face_counts, offsets(face_counts))


def save_mesh_ply(path, vertices, faces, rgb=None, normals=None) -> None:
    """Binary little-endian PLY of ONE mesh: vertices [N,3] (stored as float32), optional normals [N,3] (float32 nx, ny, nz), optional
    rgb [N,3] (uint8 as is; floats by save_ply's rule: scaled by 255 when their maximum is below 1.001), then faces [F,3] as
    `property list uchar int vertex_indices` (a count byte of 3 and three little-endian int32 per face).  Tensors or arrays; the faces
    must index the given vertices (a TriangleMesh of one volume, or one member of TriangleMesh.split())."""
    vertices, faces = _host(vertices), _host(faces)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f"save_mesh_ply: vertices must be [N,3], got {vertices.shape}")
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError(f"save_mesh_ply: faces must be an integer array [F,3], got {faces.dtype} {faces.shape}")
    if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= vertices.shape[0]):
        raise ValueError(f"save_mesh_ply: faces index outside the {vertices.shape[0]} vertices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        normals = _host(normals)
        if normals.shape != vertices.shape:
            raise ValueError(f"save_mesh_ply: normals must be [N,3] like vertices, got {normals.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb is not None:
        rgb = _rgb_u8(_host(rgb))
        if rgb.shape != vertices.shape:
            raise ValueError(f"save_mesh_ply: rgb must be [N,3] like vertices, got {rgb.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rows = np.empty(vertices.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate("xyz"):
        rows[name] = vertices[:, k]
    if normals is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            rows[name] = normals[:, k]
    if rgb is not None:
        for k, name in enumerate(("red", "green", "blue")):
            rows[name] = rgb[:, k]
    tri = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    tri["n"] = 3
    tri["v"] = faces
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {vertices.shape[0]}"]
    header += [f"property {'float' if t == '<f4' else 'uchar'} {name}" for name, t in fields]
    header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        rows.tofile(f)
        tri.tofile(f)
