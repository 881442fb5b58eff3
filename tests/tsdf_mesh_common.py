"""What the tsdf_mesh tests share (not a test module): the scenes, the call of the host program tests/tsdf_mesh_host/tsdf_mesh_host.cpp, the
numpy fp32 restatement of ud_tsdf_cell and ud_tsdf_quad (csrc/tsdf_mesh_point.h) built on tsdf_common.slots -- the restatement of the
unchanged ud_tsdf_slot -- the packing, the topology of a quad mesh and the conditions no scene set may miss.  The oracle of every test
is the restatement here, never a kernel."""
import functools

import numpy as np

import host_program
import tsdf_common as tc
from host_program import f32_bits, same_bits  # noqa: F401  (the tests reach them through this module)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------------

def cells(tsdf, weight, color, origin, voxel, min_weight):
    """ud_tsdf_cell for every cell and ud_tsdf_quad for every slot of every volume, in fp32, every operation rounded separately.
    tsdf, weight [B,Nz,Ny,Nx], color [B,3,Nz,Ny,Nx] or None, origin [1 or B,3].
    -> dict(live bool [B,n], xyz [B,n,3], rgb [B,n,3] or None, normal [B,n,3] (rows of cells that are not live are 0), slot_live bool
    [B,3n] (tsdf_points' slots), quad_live bool [B,3n], quad int32 [B,3n,4]: the four voxel indices in winding order, 0 where none)"""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    B, Nz, Ny, Nx = tsdf.shape
    n = Nz * Ny * Nx
    s_live, s_xyz, s_rgb = tc.slots(tsdf, weight, color, origin, voxel, min_weight)
    mw = np.float32(min_weight)
    iz, iy, ix = (a.reshape(-1) for a in np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij"))
    exists = (ix + 1 < Nx) & (iy + 1 < Ny) & (iz + 1 < Nz)
    lin = np.arange(n)
    stride = (1, Nx, Nx * Ny)
    t, w = tsdf.reshape(B, n), weight.reshape(B, n)
    corner = [np.minimum(lin + (c & 1) * stride[0] + ((c >> 1) & 1) * stride[1] + ((c >> 2) & 1) * stride[2], n - 1) for c in range(8)]
    d = [t[:, corner[c]] for c in range(8)]
    ok = np.broadcast_to(exists, (B, n)).copy()
    any_neg, any_pos = np.zeros((B, n), bool), np.zeros((B, n), bool)
    for c in range(8):
        ok &= (w[:, corner[c]] >= mw) & ~np.isnan(d[c])
        any_neg |= d[c] < 0
        any_pos |= ~(d[c] < 0)
    live = ok & any_neg & any_pos
    acc = np.zeros((B, n, 3), np.float32)
    cacc = np.zeros((B, n, 3), np.float32) if color is not None else None
    count = np.zeros((B, n), np.int32)
    rows = np.arange(B)[:, None]
    with np.errstate(all="ignore"):
        for e in range(12):
            axis, k = e >> 2, e & 3
            o0, o1 = [x for x in range(3) if x != axis]
            lower = np.minimum(lin + (k & 1) * stride[o0] + ((k >> 1) & 1) * stride[o1], n - 1)
            slot = 3 * lower + axis
            m = live & s_live[:, slot]
            first = (count == 0)[..., None]
            p = s_xyz[rows, slot[None]]
            acc = np.where(m[..., None], np.where(first, p, (acc + p).astype(np.float32)), acc)
            if color is not None:
                c = s_rgb[rows, slot[None]]
                cacc = np.where(m[..., None], np.where(first, c, (cacc + c).astype(np.float32)), cacc)
            count += m
        assert (count[live] >= 1).all() and (count[~live] == 0).all()
        cnt = np.where(live, count, 1).astype(np.float32)[..., None]
        xyz = np.where(live[..., None], (acc / cnt).astype(np.float32), np.float32(0))
        rgb = None if color is None else np.where(live[..., None], (cacc / cnt).astype(np.float32), np.float32(0))
        # float32 arrays throughout: numpy rounds every operation to fp32
        g = [(((d[e[1]] - d[e[0]]) + (d[e[3]] - d[e[2]])) + (d[e[5]] - d[e[4]])) + (d[e[7]] - d[e[6]])
             for e in ((0, 1, 2, 3, 4, 5, 6, 7), (0, 2, 1, 3, 4, 6, 5, 7), (0, 4, 1, 5, 2, 6, 3, 7))]
        length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        assert length.dtype == np.float32 and acc.dtype == np.float32
        good = live & (length > 0) & np.isfinite(length)
        normal = np.stack([np.where(good, x / length, np.float32(0)) for x in g], axis=-1)
    # the quads
    coord = (ix, iy, iz)
    quad_live = np.zeros((B, n, 3), bool)
    quad = np.zeros((B, n, 3, 4), np.int32)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        inside = (coord[u] >= 1) & (coord[v] >= 1)
        q0, q1, q2, q3 = (np.maximum(q, 0) for q in (lin - stride[u] - stride[v], lin - stride[v], lin, lin - stride[u]))
        m = s_live.reshape(B, n, 3)[:, :, axis] & inside & live[:, q0] & live[:, q1] & live[:, q2] & live[:, q3]
        neg = t < 0
        order = np.stack([np.broadcast_to(q0, (B, n)), np.where(neg, q1, q3), np.broadcast_to(q2, (B, n)), np.where(neg, q3, q1)], axis=-1)
        quad_live[:, :, axis] = m
        quad[:, :, axis] = np.where(m[..., None], order, 0)
    return dict(live=live, xyz=xyz, rgb=rgb, normal=normal, slot_live=s_live, quad_live=quad_live.reshape(B, 3 * n),
                quad=quad.reshape(B, 3 * n, 4))


def packed(r, rgb_u8=True):
    """cells()' arrays as tsdf_mesh packs them -> dict(vertices, faces int32 [2 * quads, 3] (rows local to the volume), rgb, normals,
    vert_counts, vert_offsets, face_counts, face_offsets, quads int32 [quads, 4] (local rows, winding order) and quad_volume [quads])"""
    live, ql = r["live"], r["quad_live"]
    vc, fc = live.sum(axis=1).astype(np.int64), 2 * ql.sum(axis=1).astype(np.int64)
    rank = np.cumsum(live, axis=1) - 1
    b = np.nonzero(ql)[0]
    q = r["quad"][ql]
    quads = rank[b[:, None], q].astype(np.int32)
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    rgb = r["rgb"]
    if rgb is not None:
        rgb = rgb[live]
        rgb = tc.to_u8(rgb) if rgb_u8 else rgb
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)  # noqa: E731
    return dict(vertices=r["xyz"][live], faces=faces, rgb=rgb, normals=r["normal"][live], vert_counts=vc, vert_offsets=off(vc), face_counts=fc,
                face_offsets=off(fc), quads=quads, quad_volume=b)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------

GRID, VOXEL, TRUNC = (11, 13, 9), 0.1, 0.25                                    # (Nz, Ny, Nx)
CENTRE, RADIUS = (0.47, 0.66, 0.52), 0.31
# two spheres more than two voxels apart, their centres off the lattice of voxel centres (a centre ON it makes crossings coincide: triangles
# of no area, which have no normal to test)
PAIR = (((0.27, 0.34, 0.31), 0.17), ((0.61, 0.93, 0.77), 0.21))
# Zeroing a random tenth of the weights keeps a cell live with probability 0.9^8 = 0.43, about 8 % of the cells of the sphere scene: most
# draws miss the 10 % that assert_not_vacuous asks of every scene.  This draw keeps 98 of the 960 cells (78 referenced, 41 quads of 153 slots).
HOLE_SEED = 33


def _centres(grid, voxel):
    Nz, Ny, Nx = grid
    z, y, x = np.meshgrid(*(((np.arange(n) + 0.5) * voxel) for n in (Nz, Ny, Nx)), indexing="ij")
    return x, y, z


def sphere_field(spheres, grid=GRID, voxel=VOXEL, trunc=TRUNC):
    """the truncated distance to the nearest of the spheres ((cx, cy, cz), r), negative inside, the origin at 0 -> fp32 [1,Nz,Ny,Nx]"""
    x, y, z = _centres(grid, voxel)
    dist = np.min([np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r for c, r in spheres], axis=0)
    return np.clip(dist / trunc, -1, 1).astype(np.float32)[None]


@functools.lru_cache(maxsize=None)
def scene(name):
    """name -> read-only dict(tsdf, weight [B,Nz,Ny,Nx], color [B,3,Nz,Ny,Nx], origin [1 or B,3], voxel, min_weight).
    sphere, pair (two disjoint spheres), hole (the sphere with a random tenth of the weights zeroed), random (a normal field: nearly
    every cell live), special (the sphere with +-inf, -0.0, NaN and exact zeros planted along its surface)."""
    g = np.random.RandomState(4100)
    t = sphere_field(((CENTRE, RADIUS),))
    w = np.ones_like(t)
    if name == "pair":
        t = sphere_field(PAIR)
    elif name == "hole":
        gh = np.random.RandomState(HOLE_SEED)
        flat = w.reshape(-1)
        flat[gh.permutation(flat.size)[:flat.size // 10]] = 0
    elif name == "random":
        t = g.normal(size=t.shape).astype(np.float32)
    elif name == "special":
        t = t.copy()
        near = np.argwhere(np.abs(t[0]) < 0.5)                                 # voxels next to the surface, where a value changes the mesh
        pick = near[g.permutation(len(near))[:48]]
        values = [np.inf, -np.inf, -0.0, 0.0, np.nan, 0.0, -0.0, np.float32(1e-45)]
        for k, (z, y, x) in enumerate(pick):
            t[0, z, y, x] = values[k % len(values)]
    elif name != "sphere":
        raise ValueError(name)
    c = g.uniform(0, 255, size=(1, 3) + t.shape[1:]).astype(np.float32)
    d = dict(tsdf=t, weight=w, color=c, origin=np.zeros((1, 3), np.float32), voxel=tc.f32(VOXEL), min_weight=1.0)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


SCENES = ("sphere", "pair", "hole", "random", "special")


@functools.lru_cache(maxsize=None)
def restated(name):
    s = scene(name)
    return cells(s["tsdf"], s["weight"], s["color"], s["origin"], s["voxel"], s["min_weight"])


def plane(grid, below_positive, layer=0):
    """a flat surface between the z layers `layer` and `layer + 1`; the positive side below or above -> tsdf, weight [1,Nz,Ny,Nx]"""
    Nz, Ny, Nx = grid
    t = np.empty((1, Nz, Ny, Nx), np.float32)
    t[:, :layer + 1] = 0.5 if below_positive else -0.5
    t[:, layer + 1:] = -0.5 if below_positive else 0.5
    return t, np.ones_like(t)


def batch(names, per_origin=False):
    """scenes of one grid stacked into a batch -> the arrays of scene(); per_origin: every volume's origin moved by a fraction of a voxel"""
    ss = [scene(nm) for nm in names]
    o = np.zeros((1, 3), np.float32)
    if per_origin:
        o = np.stack([np.float32(0.37 * VOXEL * b) * np.ones(3, np.float32) for b in range(len(ss))]).astype(np.float32)
    return dict(tsdf=np.concatenate([s["tsdf"] for s in ss]), weight=np.concatenate([s["weight"] for s in ss]),
                color=np.concatenate([s["color"] for s in ss]), origin=o, voxel=ss[0]["voxel"], min_weight=1.0)


# ---- the host program -------------------------------------------------------------------------------------------------------------

def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "tsdf_mesh_host")


def host_cells(exe, tsdf, weight, color, origin, voxel, min_weight):
    """tests/tsdf_mesh_host on a volume: ud_tsdf_cell for every cell and ud_tsdf_quad for every slot -> cells()' dict, with rgb_u8 beside
    rgb (the program exits with 3 when a predicate depends on whether the payload is asked for)"""
    tsdf = np.ascontiguousarray(tsdf, np.float32)
    B, Nz, Ny, Nx = tsdf.shape
    n = Nz * Ny * Nx
    origin = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
    has_color = color is not None
    blobs = [tsdf.tobytes(), np.ascontiguousarray(weight, np.float32).tobytes()]
    blobs += [np.ascontiguousarray(color, np.float32).tobytes()] if has_color else []
    blobs += [origin.tobytes()]
    args = [B, Nz, Ny, Nx, origin.shape[0], int(has_color), f32_bits(voxel), f32_bits(min_weight)]
    c = B * n * 3 if has_color else 0
    parts = host_program.run(exe, args, blobs, [B * n, 12 * B * n, 12 * B * n, 4 * c, c, 3 * B * n, 4 * 4 * 3 * B * n])
    return dict(live=np.frombuffer(parts[0], np.uint8).reshape(B, n).astype(bool), xyz=np.frombuffer(parts[1], np.float32).reshape(B, n, 3),
                normal=np.frombuffer(parts[2], np.float32).reshape(B, n, 3),
                rgb=np.frombuffer(parts[3], np.float32).reshape(B, n, 3) if has_color else None,
                rgb_u8=np.frombuffer(parts[4], np.uint8).reshape(B, n, 3) if has_color else None,
                quad_live=np.frombuffer(parts[5], np.uint8).reshape(B, 3 * n).astype(bool),
                quad=np.frombuffer(parts[6], np.int32).reshape(B, 3 * n, 4))


def assert_same_cells(got, want, what=""):
    for k in ("live", "xyz", "normal", "rgb", "quad_live", "quad"):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert same_bits(got[k], want[k]), (what, k, int((np.asarray(got[k]).view(np.uint8) != np.asarray(want[k]).view(np.uint8)).sum()))


# ---- topology and the conditions no scene set may miss ------------------------------------------------------------------------------

def topology(quads, n_vertices):
    """quads int [Q,4] in winding order -> dict(V, E, F, euler, closed: every undirected edge in exactly two quads, wound: no directed
    edge twice, oriented: wound and every directed edge's reverse present, referenced: the vertices some quad uses)"""
    a, b = quads.reshape(-1), np.roll(quads, -1, axis=1).reshape(-1)
    directed = a.astype(np.int64) * max(n_vertices, 1) + b
    und = np.minimum(a, b).astype(np.int64) * max(n_vertices, 1) + np.maximum(a, b)
    _, per_edge = np.unique(und, return_counts=True)
    uniq = np.unique(directed)
    reverse = b.astype(np.int64) * max(n_vertices, 1) + a
    return dict(V=n_vertices, E=len(per_edge), F=len(quads), euler=n_vertices - len(per_edge) + len(quads), closed=bool((per_edge == 2).all()),
                wound=len(uniq) == len(directed), oriented=len(uniq) == len(directed) and bool(np.isin(reverse, uniq).all()),
                referenced=np.unique(quads))


def windings(r):
    """per axis (quads wound (q0, q1, q2, q3), quads wound (q0, q3, q2, q1)) of cells()' result"""
    ql, q = r["quad_live"].reshape(-1, 3), r["quad"].reshape(-1, 3, 4)
    out = []
    for axis in range(3):
        qa = q[:, axis][ql[:, axis]]
        forward = qa[:, 1] > qa[:, 3] if axis == 1 else qa[:, 1] < qa[:, 3]      # q1 = c - e_v, q3 = c - e_u: e_v > e_u except for the y axis
        out.append((int(forward.sum()), int((~forward).sum())))
    return out


def live_share(s, r):
    B, Nz, Ny, Nx = s["tsdf"].shape
    return float(r["live"].sum()) / (B * (Nz - 1) * (Ny - 1) * (Nx - 1))


def assert_not_vacuous(name, s, r):
    """between 10 % and 90 % of the existing cells live (the random field is exempt: nearly all of its cells are live by construction and
    it must only match bits) and both windings on each of the three axes"""
    if name == "random":
        return
    share = live_share(s, r)
    assert 0.1 <= share <= 0.9, (name, share)
    for axis, (f, bwd) in enumerate(windings(r)):
        assert f > 0 and bwd > 0, (name, axis, f, bwd)
