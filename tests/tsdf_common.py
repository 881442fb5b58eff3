"""What the tsdf tests share (not a test module): the scenes -- a plane at z = 2 with a block at 1.7 and holes, seen by V views through any
of the six camera models -- the call of the host program tests/tsdf_host/tsdf_host.cpp, the numpy fp32 restatement of ud_tsdf_slot
(csrc/tsdf_point.h), the conditions no scene may miss, the known answer and the special values.  The oracle of the GPU integration tests
is unidepth_amd.tsdf.tsdf_integrate_composition, the merged calls in a loop, never the fused kernel; the oracle of tsdf_points is the
restatement here."""
import functools

import numpy as np

import host_program
from host_program import ROOT, bits, f32_bits  # noqa: F401  (the tests reach them through this module)

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = 1, 2, 3, 4, 5, 6
MODELS = (PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI)
NAMES = {PINHOLE: "pinhole", EUCM: "eucm", SPHERICAL: "spherical", OPENCV: "opencv", FISHEYE624: "fisheye624", MEI: "mei"}
MAX_WEIGHT = 1.5                                              # below the weight three views add up to, so the clamp acts
# (Nz, Ny, Nx), voxel size, origin, trunc: the base scene (2457 voxels: nine full workgroups and a partial one) and a coarser second one
BASE = dict(grid=(9, 13, 21), voxel=0.1, origin=(-1.05, -0.65, 1.5), trunc=0.3)
SECOND = dict(grid=(5, 7, 13), voxel=0.2, origin=(-1.3, -0.7, 1.7), trunc=0.4)


def f32(x):
    return float(np.float32(x))


def row_for(model, Hs, Ws, f):
    """one 16-float parameter row of `model` for an Hs x Ws view whose pinhole focal length would be f, centre in the middle"""
    cx, cy = Ws / 2, Hs / 2
    row = np.zeros(16, np.float32)
    if model == PINHOLE:
        row[:4] = [f, f, cx, cy]
    elif model == EUCM:
        row[:6] = [f, f, cx, cy, 0.5, 1.0]
    elif model == SPHERICAL:
        hfov = np.arctan((Ws / 2) / f)
        row[:8] = [f, f, cx, cy, max(Ws, 2), max(Hs, 2), hfov, np.arctan(np.tan(hfov) * Hs / Ws)]   # the model divides by W - 1 and H - 1
    elif model == OPENCV:
        row[:4] = [f, f, cx, cy]
        row[4:7] = [-0.05, 0.01, -0.001]
        row[10:16] = [1e-3, -1e-3, 2e-3, 1e-4, -1e-3, 2e-4]
    elif model == FISHEYE624:
        row[:4] = [1.2 * f, 1.2 * f, cx, cy]
        row[4:10] = [-0.02, 0.004, -0.001, 2e-4, -1e-4, 1e-5]
        row[10:16] = [1e-3, -1e-3, 2e-3, 1e-4, -1e-3, 2e-4]
    elif model == MEI:
        row[:9] = [1.9 * f, 1.9 * f, cx, cy, -0.05, 0.01, 1e-3, -1e-3, 0.9]
    else:
        raise ValueError(model)
    return row


def _rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


@functools.lru_cache(maxsize=None)
def scene(models, B=2, V=3, Hs=11, Ws=19, grid=BASE["grid"], voxel=BASE["voxel"], origin=BASE["origin"], trunc=BASE["trunc"],
          per_image=False, per_origin=False, seed=0):
    """numpy, read-only.  models: one tag for every view of every image, or a tuple models[v][b].  Every view looks along +z from
    x = -0.3 .. +0.3 (spread evenly over the views) at the plane z = 2, with the block [Hs/3:2Hs/3, Ws/3:Ws/2] at 1.7 and a random tenth
    of the pixels set to 0.  depths [B,V,Hs,Ws]; src_masks (8 % zeros), src_weights (0.5 .. 1.5), images uint8 [B,V,3,Hs,Ws]; params
    [V,B,16]; T [V,3,4] (shared) or [B,V,3,4] (per_image: the poses of the other images turned by up to 0.03 rad); origin [1,3] or [B,3]
    (per_origin: moved by a fraction of a voxel per image)."""
    g = np.random.RandomState(9600 + seed)
    if isinstance(models, int):
        models = ((models,) * B,) * V
    f = 9.0 * Ws / 19.0
    params = np.stack([np.stack([row_for(models[v][b], Hs, Ws, f) for b in range(B)]) for v in range(V)])
    xs = np.linspace(-0.3, 0.3, V) if V > 1 else np.zeros(1)

    def pose(v, b):
        R = _rot(g.normal(size=3), g.uniform(-0.03, 0.03)) if (per_image and b > 0) else np.eye(3)
        c = np.array([xs[v], 0.0, 0.0])
        return np.concatenate([R, (-R @ c)[:, None]], axis=1).astype(np.float32)
    T = np.stack([np.stack([pose(v, b) for v in range(V)]) for b in range(B)]) if per_image else np.stack([pose(v, 0) for v in range(V)])
    depths = np.full((B, V, Hs, Ws), 2.0, np.float32)
    depths[:, :, Hs // 3:2 * Hs // 3, Ws // 3:Ws // 2] = 1.7
    depths[g.uniform(size=depths.shape) < 0.1] = 0.0
    o = np.array(origin, np.float32)[None]
    if per_origin:
        o = np.stack([o[0] + np.float32(0.37 * voxel * b) for b in range(B)]).astype(np.float32)
    d = dict(B=B, V=V, Hs=Hs, Ws=Ws, grid=tuple(grid), voxel=f32(voxel), trunc=f32(trunc), origin=o, depths=depths,
             src_masks=(g.uniform(size=depths.shape) >= 0.08).astype(np.uint8), src_weights=g.uniform(0.5, 1.5, size=depths.shape).astype(np.float32),
             images=g.randint(0, 256, size=(B, V, 3, Hs, Ws)).astype(np.uint8), models=tuple(tuple(r) for r in models), params=params, T=T)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def mixed_models(B=2, V=3):
    """models[v][b]: all six models in one batch of B = 2 images and V = 3 views"""
    return tuple(tuple(MODELS[(v * B + b) % 6] for b in range(B)) for v in range(V))


# name -> scene arguments: rows of voxels around the wave's and the workgroup's edges, a single voxel, tiny views, one view, and
# B * V = 256 on a 3x3x3 grid.  The rows lie just in front of the plane (behind the block) and are 8 units long, wider than any view sees.
def _row(nx, ny, nz):
    vox = 8.0 / max(nx, 8)
    return dict(models=mixed_models(), grid=(nz, ny, nx), voxel=vox, origin=(-nx * vox / 2, -ny * vox / 2, 1.8),
                trunc=0.3)


EDGES = {f"nx{nx}_{ny}_{nz}": _row(nx, ny, nz) for nx, ny, nz in ((1, 1, 2), (63, 2, 1), (64, 1, 2), (65, 2, 2), (255, 1, 1), (257, 2, 1))}
EDGES.update({"one_voxel": dict(models=mixed_models(), grid=(1, 1, 1), voxel=0.1, origin=(-0.05, -0.05, 1.9), trunc=0.3),
              "src1x1": dict(models=mixed_models(), Hs=1, Ws=1), "src2x3": dict(models=mixed_models(), Hs=2, Ws=3),
              "v1": dict(models=mixed_models(V=1), V=1),
              "limit": dict(models=tuple(tuple(MODELS[(v + b) % 6] for b in range(32)) for v in range(8)), B=32, V=8, grid=(3, 3, 3), voxel=0.25,
                            origin=(-0.375, -0.375, 1.875), trunc=0.3)})
# the scenes too small to have a share: some voxel is updated by some view and (more than one decision) some decision is false
TINY = ("nx1_1_2", "one_voxel")


def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "tsdf_host")


def host_tsdf(exe, s, *, src_masks=False, src_weights=False, images=False, max_weight=None, volume=None, min_weight=1.0, views=None):
    """tests/tsdf_host on the scene s (the optional inputs by flag; `views` a slice of the views; volume = (tsdf, weight, color or None) to
    continue from), after the program has checked ud_tsdf_voxel against the chain of the separate functions (exit status 3 when they
    differ, a sanitizer report otherwise).
    -> dict(tsdf, weight [B,Nz,Ny,Nx], color [B,3,Nz,Ny,Nx] or None, count uint8, and of the resulting volume at min_weight: live bool
    [B,3n], xyz [B,3n,3], rgb_f32 / rgb_u8 [B,3n,3] or None)"""
    vsel = slice(None) if views is None else views
    depths = np.ascontiguousarray(s["depths"][:, vsel])
    B, V, Hs, Ws = depths.shape
    Nz, Ny, Nx = s["grid"]
    n = Nz * Ny * Nx
    T = np.ascontiguousarray(s["T"].reshape(-1, s["V"], 3, 4)[:, vsel])
    params = np.ascontiguousarray(s["params"][vsel])
    models = s["models"][vsel]
    blobs = [depths.tobytes()]
    blobs += [np.ascontiguousarray(s["src_masks"][:, vsel]).tobytes()] if src_masks else []
    blobs += [np.ascontiguousarray(s["src_weights"][:, vsel]).tobytes()] if src_weights else []
    blobs += [np.ascontiguousarray(s["images"][:, vsel]).tobytes()] if images else []
    blobs += [params.tobytes(), T.tobytes(), np.ascontiguousarray(s["origin"], np.float32).tobytes()]
    if volume is not None:
        blobs += [np.ascontiguousarray(volume[0], np.float32).tobytes(), np.ascontiguousarray(volume[1], np.float32).tobytes()]
        blobs += [np.ascontiguousarray(volume[2], np.float32).tobytes()] if images else []
    args = [B, V, Nz, Ny, Nx, Hs, Ws, T.shape[0], s["origin"].shape[0], int(src_masks), int(src_weights), int(images), int(volume is None),
            int(max_weight is not None), f32_bits(s["voxel"]), f32_bits(s["trunc"]), f32_bits(max_weight or 0.0), f32_bits(min_weight)]
    args += [models[v][b] for v in range(V) for b in range(B)]
    c = 3 * n * B if images else 0
    S = 3 * n * B
    parts = host_program.run(exe, args, blobs, [4 * n * B, 4 * n * B, 4 * c, n * B, S, 12 * S, 12 * S if images else 0, 3 * S if images else 0])
    shape = (B, Nz, Ny, Nx)
    return dict(min_weight=min_weight, tsdf=np.frombuffer(parts[0], np.float32).reshape(shape), weight=np.frombuffer(parts[1], np.float32).reshape(shape),
                color=np.frombuffer(parts[2], np.float32).reshape(B, 3, Nz, Ny, Nx) if images else None,
                count=np.frombuffer(parts[3], np.uint8).reshape(shape), live=np.frombuffer(parts[4], np.uint8).reshape(B, 3 * n).astype(bool),
                xyz=np.frombuffer(parts[5], np.float32).reshape(B, 3 * n, 3),
                rgb_f32=np.frombuffer(parts[6], np.float32).reshape(B, 3 * n, 3) if images else None,
                rgb_u8=np.frombuffer(parts[7], np.uint8).reshape(B, 3 * n, 3) if images else None)


# ---- the numpy restatement of ud_tsdf_slot ----------------------------------------------------------------------------------------------

def slots(tsdf, weight, color, origin, voxel, min_weight):
    """csrc/tsdf_point.h's ud_tsdf_slot for every slot s = 3 * voxel + axis of every volume, in fp32, every operation rounded separately.
    tsdf, weight [B,Nz,Ny,Nx], color [B,3,Nz,Ny,Nx] or None, origin [1 or B,3].
    -> live bool [B,3n], xyz fp32 [B,3n,3], rgb fp32 [B,3n,3] or None (rows of slots that are not live are 0)"""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    B, Nz, Ny, Nx = tsdf.shape
    n = Nz * Ny * Nx
    vs, mw = np.float32(voxel), np.float32(min_weight)
    o = np.broadcast_to(np.asarray(origin, np.float32).reshape(-1, 3), (B, 3))
    iz, iy, ix = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    idx = (ix, iy, iz)
    centre = [o[:, k].reshape(B, 1, 1, 1) + ((idx[k].astype(np.float32) + np.float32(0.5)) * vs)[None] for k in range(3)]
    live = np.zeros((B, n, 3), bool)
    xyz = np.zeros((B, n, 3, 3), np.float32)
    rgb = np.zeros((B, n, 3, 3), np.float32) if color is not None else None
    with np.errstate(all="ignore"):
        for axis, dim in enumerate((3, 2, 1)):                                  # +x, +y, +z: the neighbour along the last, middle, first grid axis
            def nb(a, d=dim):
                """the +axis neighbour's value, with the last layer (no neighbour) repeated: those slots are not live"""
                return np.concatenate([np.take(a, range(1, a.shape[d]), axis=d), np.take(a, [a.shape[d] - 1], axis=d)], axis=d)
            in_grid = np.broadcast_to(idx[axis] + 1 < (Nx, Ny, Nz)[axis], tsdf.shape)
            a, b = tsdf, nb(tsdf)
            ok = in_grid & (weight >= mw) & (nb(weight) >= mw) & ~np.isnan(a) & ~np.isnan(b) & ((a < 0) != (b < 0))
            t = (a / (a - b)).astype(np.float32)
            p = [c.copy() for c in centre]
            p[axis] = (p[axis] + (t * vs).astype(np.float32)).astype(np.float32)
            live[:, :, axis] = ok.reshape(B, n)
            for k in range(3):
                xyz[:, :, axis, k] = np.where(ok, p[k], np.float32(0)).reshape(B, n)
            if color is not None:
                col = np.asarray(color, np.float32)
                for k in range(3):
                    c0, c1 = col[:, k], nb(col[:, k], dim)
                    rgb[:, :, axis, k] = np.where(ok, c0 + (t * (c1 - c0)).astype(np.float32), np.float32(0)).reshape(B, n)
    return live.reshape(B, 3 * n), xyz.reshape(B, 3 * n, 3), None if rgb is None else rgb.reshape(B, 3 * n, 3)


def to_u8(x):
    """remap_taps.h's ud_rm_to_u8: round half to even, clamp to [0, 255], NaN -> 0"""
    r = np.rint(np.asarray(x, np.float32))
    return np.where(r >= 0, np.where(r <= 255, r, 255), 0).astype(np.uint8)


def planted(B, grid, seed, empty=None):
    """B volumes of grid = (Nz, Ny, Nx) voxels with random distances (a few NaN), weights in {0, 1, 2}, colours and origins; volume
    `empty` has no weight -> tsdf, weight [B,Nz,Ny,Nx], color [B,3,Nz,Ny,Nx], origin [B,3]"""
    g = np.random.RandomState(9700 + seed)
    t = g.uniform(-1, 1, size=(B,) + tuple(grid)).astype(np.float32)
    t[g.uniform(size=t.shape) < 0.03] = np.nan
    w = g.randint(0, 3, size=t.shape).astype(np.float32)
    if empty is not None:
        w[empty] = 0
    c = g.uniform(0, 255, size=(B, 3) + tuple(grid)).astype(np.float32)
    o = g.uniform(-1, 1, size=(B, 3)).astype(np.float32)
    return t, w, c, o


MANY_TILES_GRID = (16, 8, 683)     # 87,424 voxels, 262,272 slots = 257 tiles of 1024: the scan of one volume's tile counts needs its carry


def many_tiles_volumes():
    """two different volumes of MANY_TILES_GRID whose restatement has live slots in the tiles 0, 255 (the last of the scan's first
    chunk of 256), 256 (the second chunk, a partial tile) -> planted()'s arrays and the voxel size"""
    vol = planted(2, MANY_TILES_GRID, 257)
    live = slots(vol[0], vol[1], None, vol[3], f32(0.05), 1.0)[0]
    assert live.shape == (2, 262272)
    per_tile = np.add.reduceat(live, np.arange(0, live.shape[1], 1024), axis=1)
    assert per_tile.shape == (2, 257) and (per_tile[:, (0, 255, 256)] > 0).all(), per_tile[:, (0, 255, 256)]
    assert (per_tile[0] != per_tile[1]).any()
    return vol, f32(0.05)


def packed(live, xyz, rgb):
    """the slot arrays as tsdf_points packs them -> xyz [total,3], rgb [total,3] or None, counts int64 [B], offsets int64 [B+1]"""
    counts = live.sum(axis=1).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return xyz[live], None if rgb is None else rgb[live], counts, offsets


# ---- the conditions no scene may miss ----------------------------------------------------------------------------------------------

def view_counts(exe, s, **kw):
    """count [V][B,Nz,Ny,Nx]: each view integrated alone into a fresh volume"""
    return [host_tsdf(exe, s, views=slice(v, v + 1), **kw)["count"] for v in range(s["V"])]


def assert_not_vacuous(name, r, per_view):
    """r: host_tsdf's result over all views; per_view: view_counts'.  Each view updates strictly between 10 % and 90 % of the voxels; at
    least 10 % of the voxels end inside the band |tsdf| < 1; the live slots are more than 0 and fewer than half of all."""
    if name in TINY:
        assert r["count"].any() and (r["count"][0].size == 1 or not (r["count"] == len(per_view)).all()), name
        return
    shares = [float(c.astype(bool).mean()) for c in per_view]
    assert min(shares) > 0.1 and max(shares) < 0.9, (name, shares)
    band = float((np.abs(r["tsdf"]) < 1).mean())
    assert band >= 0.1, (name, band)
    n_live = int(r["live"].sum())
    assert 0 < n_live < r["live"].size / 2, (name, n_live)


# ---- the known answer ----------------------------------------------------------------------------------------------------------------

def known_answer_scene():
    """One Pinhole view at the volume's origin looking along +z (identity transform) at a constant depth of 2; voxel 0.25, trunc 0.5 and an
    origin that puts every centre on a multiple of 0.125: every intermediate is exact in fp32."""
    Hs = Ws = 16
    row = np.zeros((1, 1, 16), np.float32)
    row[..., :4] = [8.0, 8.0, 8.0, 8.0]
    T = np.zeros((1, 3, 4), np.float32)
    T[0, :, :3] = np.eye(3)
    return dict(B=1, V=1, Hs=Hs, Ws=Ws, grid=(12, 4, 4), voxel=0.25, trunc=0.5, origin=np.array([[-0.5, -0.5, 0.5]], np.float32),
                depths=np.full((1, 1, Hs, Ws), 2.0, np.float32), models=((PINHOLE,),), params=row, T=T)


def check_known_answer(tsdf, weight, count, live, xyz):
    """tsdf = min(1, (2 - z) / 0.5) exactly where 2 - z >= -0.5, untouched (1, weight 0) behind that; every surface point has z == 2.0"""
    s = known_answer_scene()
    Nz, Ny, Nx = s["grid"]
    z = np.float32(0.5) + (np.arange(Nz, dtype=np.float32) + np.float32(0.5)) * np.float32(0.25)         # 0.625 .. 3.375
    seen = (np.float32(2.0) - z) >= np.float32(-0.5)
    want = np.where(seen, np.minimum(np.float32(1), (np.float32(2.0) - z) / np.float32(0.5)), np.float32(1)).astype(np.float32)
    assert seen.any() and not seen.all() and (want < 0).any() and ((want > 0) & (want < 1)).any()
    full = np.broadcast_to(want[None, :, None, None], tsdf.shape)
    assert host_program.same_bits(np.ascontiguousarray(tsdf), np.ascontiguousarray(full))
    assert np.array_equal(weight, np.broadcast_to(seen[None, :, None, None].astype(np.float32), weight.shape))
    assert np.array_equal(count, np.broadcast_to(seen[None, :, None, None].astype(np.uint8), count.shape))
    pts = xyz[live]
    assert len(pts) == Ny * Nx and (pts[:, 2] == np.float32(2.0)).all()                                    # one +z crossing per column
    assert set(np.unique(pts[:, 0]).tolist()) == {-0.375, -0.125, 0.125, 0.375}


# ---- special values ------------------------------------------------------------------------------------------------------------------

def special_scene():
    """the per-image base scene of a mixed batch of three images with: NaN, +-inf, 0, -0.0 and negative values spread over the depths; NaN,
    0, inf and negative values over the weights; image 1's views singular Pinholes (fx = 0); image 2's transforms turned so that every
    voxel lies behind every view"""
    models = tuple(tuple(PINHOLE if b == 1 else MODELS[(v * 3 + b) % 6] for b in range(3)) for v in range(3))
    s = dict(scene(models, B=3, per_image=True, seed=5))
    depths, weights, params, T = np.array(s["depths"]), np.array(s["src_weights"]), np.array(s["params"]), np.array(s["T"])
    depths[:, :, ::3, ::4] = np.nan
    depths[:, :, 1::3, 1::4] = np.inf
    depths[:, :, 2::3, 2::4] = -np.inf
    depths[:, :, 2::3, 3::4] = -0.0
    depths[:, :, 1::3, 2::4] = -2.0
    weights[:, :, ::2, ::5] = np.nan
    weights[:, :, 1::2, 1::5] = 0.0
    weights[:, :, ::2, 2::5] = np.inf
    weights[:, :, 1::2, 3::5] = -1.0
    params[:, 1, 0] = 0.0
    T[2, :, 2, :] = [0.0, 0.0, -1.0, 0.0]                                       # z' = -z for every voxel of image 2
    s.update(depths=depths, src_weights=weights, params=params, T=T)
    return s


def check_special(r, s, weights):
    """what must hold of any result on special_scene(): no voxel is updated that its inputs cannot support"""
    assert not r["count"][2].any() and (r["tsdf"][2] == 1).all() and (r["weight"][2] == 0).all()            # behind every view
    assert r["count"][0].any()                                                                              # image 0 is an ordinary one
    touched = r["count"] > 0
    # an infinite depth is a surface infinitely far behind the voxel: tsdf 1; nothing else leaves [-1, 1] or the finite numbers
    assert np.isfinite(r["tsdf"]).all() and (np.abs(r["tsdf"]) <= 1).all()
    assert np.isfinite(r["weight"]).all() and (r["weight"][touched] > 0).all() and (r["weight"][~touched] == 0).all()
    assert (r["tsdf"][~touched] == 1).all()
    assert (r["count"] <= s["V"]).all()
    if not weights:
        assert np.array_equal(r["weight"], r["count"].astype(np.float32))


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------

def prepared(params, models):
    """a PreparedCamera on the GPU from numpy rows and model tags"""
    import torch
    from unidepth_amd import gtpoints
    return gtpoints.PreparedCamera(torch.from_numpy(np.array(params, np.float32, order="C")).cuda(), models)


OUTPUTS = ("tsdf", "weight", "color", "count")
