"""What the tsdf_render tests share (not a test module): the volumes -- tsdf_common's scenes integrated by its host program -- the render
poses, the call of the host program tests/tsdf_render_host/tsdf_render_host.cpp, the numpy fp32 restatement of the FULL scan of
csrc/tsdf_ray.h's ud_tsdf_ray (it takes the directions as input: numpy cannot restate Spherical's sinf / cosf bit for bit), the conditions
no scene may miss, the known answer and the special values.  The oracle of the GPU tests is the restatement on the rays form, never the
fused kernel."""
import functools

import numpy as np

import host_program
import tsdf_common as tc
from host_program import f32_bits, same_bits  # noqa: F401

CLOSED = (tc.PINHOLE, tc.EUCM, tc.SPHERICAL, tc.MEI)
SIZE = (11, 19)
NEAR, FAR = 0.5, 3.25
OUTPUTS = ("depth", "valid", "points", "normals", "color")
F = np.float32


def build_hosts(tmp_path_factory):
    """(the integration program of tsdf_common, the render program)"""
    return tc.build_host(tmp_path_factory), host_program.build(tmp_path_factory, "tsdf_render_host")


def invert(T):
    """numpy [..,3,4] rigid motions inverted as consistency.invert_rigid does, in fp32"""
    T = np.asarray(T, F)
    R, t = T[..., :3, :3], T[..., :3, 3]
    Rt = np.swapaxes(R, -1, -2)
    ti = -((Rt[..., :, 0] * t[..., 0:1] + Rt[..., :, 1] * t[..., 1:2]) + Rt[..., :, 2] * t[..., 2:3])
    return np.concatenate([Rt, ti[..., None]], axis=-1).astype(F)


def pose(eye, target, roll=0.0):
    """VOLUME TO CAMERA [3,4] of a camera at `eye` looking at `target` (x right, y down, z forward)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, -1.0, 0.0], z)
    x = -x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z]) if roll == 0.0 else tc._rot([0, 0, 1], roll) @ np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], axis=1).astype(F)


# the poses of a batch of two, both from the side at the height of the block: some rays meet the plane from the front, some run through
# the band behind the block into the free space beside it (a back crossing), and the outer ones pass the volume
POSES = (pose((-1.5, -0.3, 1.6), (0.1, 0.0, 2.05)), pose((1.2, -0.3, 1.6), (-0.3, 0.0, 1.8)))


def transforms(per_image, B=2):
    """volume to camera: [1,3,4] shared, or [B,3,4]"""
    return np.stack([POSES[b % 2] for b in range(B)]) if per_image else POSES[0][None].copy()


@functools.lru_cache(maxsize=None)
def _volume(exe, colour, second, per_origin, seed=0):
    s = tc.scene(tc.mixed_models(), per_origin=per_origin, seed=seed, **(tc.SECOND if second else tc.BASE))
    r = tc.host_tsdf(exe, s, images=colour, src_weights=True)
    return dict(tsdf=r["tsdf"], weight=r["weight"], color=r["color"], origin=np.array(s["origin"], F), voxel=s["voxel"], grid=s["grid"], B=s["B"])


def volume(exe, colour=True, second=False, per_origin=False, seed=0):
    """tsdf_common's BASE (9 x 13 x 21) or SECOND scene, B = 2, three views of all six models with per-pixel weights (0.5 .. 1.5, so a
    min_weight of 1 cuts into it), integrated by tests/tsdf_host -> dict(tsdf, weight [B,Nz,Ny,Nx], color or None, origin, voxel, grid, B)"""
    return _volume(exe, colour, second, per_origin, seed)


def planted(grid, voxel, origin, B=1, plane=None):
    """a volume whose distance is plane - z of the voxel centre (plane defaults to the middle), weight 2, colours a ramp"""
    Nz, Ny, Nx = grid
    o = np.array(origin, F).reshape(1, 3)
    z = o[0, 2] + (np.arange(Nz, dtype=F) + F(0.5)) * F(voxel)
    plane = F(o[0, 2] + F(voxel) * F(Nz) / F(2)) if plane is None else F(plane)
    t = np.broadcast_to((plane - z)[None, :, None, None], (B, Nz, Ny, Nx)).astype(F)
    c = np.broadcast_to(np.arange(Nx, dtype=F)[None, None, None, None] * F(10), (B, 3, Nz, Ny, Nx)).astype(F)
    return dict(tsdf=t, weight=np.full(t.shape, 2, F), color=c, origin=o, voxel=tc.f32(voxel), grid=tuple(grid), B=B)


def params_for(models, size, focal=14.0):
    Ho, Wo = size
    return np.stack([tc.row_for(m, Ho, Wo, focal * Wo / 19.0 if Wo >= 8 else focal) for m in models]).astype(F)


def n_samples(near, far, step):
    near, far, step = (float(F(v)) for v in (near, far, step))
    return int(np.floor((far - near) / step)) + 1


def host_render(exe, vol, models, params, size, T_cv=None, rays=None, near=NEAR, far=FAR, step=None, min_weight=1.0, colour=True):
    """tests/tsdf_render_host on a volume (T_cv: CAMERA TO VOLUME [nT,3,4] or None), after the program has compared the clipped with the
    full scan (exit status 3 when they differ, a sanitizer report otherwise) -> dict(dirs, depth, valid, points, normals, color_f32,
    color_u8 or None)"""
    B, (Nz, Ny, Nx), (Ho, Wo) = vol["B"], vol["grid"], size
    hw = Ho * Wo
    colour = colour and vol["color"] is not None
    step = vol["voxel"] if step is None else step
    K = n_samples(near, far, step)
    blobs = [np.ascontiguousarray(vol["tsdf"], F).tobytes(), np.ascontiguousarray(vol["weight"], F).tobytes()]
    blobs += [np.ascontiguousarray(vol["color"], F).tobytes()] if colour else []
    blobs += [np.ascontiguousarray(vol["origin"], F).tobytes()]
    blobs += [np.ascontiguousarray(T_cv, F).tobytes()] if T_cv is not None else []
    blobs += [np.ascontiguousarray(params, F).tobytes()]
    blobs += [np.ascontiguousarray(rays, F).tobytes()] if rays is not None else []
    args = [B, Ho, Wo, Nz, Ny, Nx, 0 if T_cv is None else len(T_cv), len(vol["origin"]), int(colour), int(rays is not None), K,
            f32_bits(vol["voxel"]), f32_bits(near), f32_bits(step), f32_bits(min_weight)] + list(models)
    c = B * 3 * hw if colour else 0
    p = host_program.run(exe, args, blobs, [12 * B * hw, 4 * B * hw, B * hw, 12 * B * hw, 12 * B * hw, 4 * c, c])
    f = lambda k, shape: np.frombuffer(p[k], F).reshape(shape)       # noqa: E731
    return dict(dirs=f(0, (B, 3, Ho, Wo)), depth=f(1, (B, 1, Ho, Wo)), valid=np.frombuffer(p[2], np.uint8).reshape(B, 1, Ho, Wo).astype(bool),
                points=f(3, (B, 3, Ho, Wo)), normals=f(4, (B, 3, Ho, Wo)), color_f32=f(5, (B, 3, Ho, Wo)) if colour else None,
                color_u8=np.frombuffer(p[6], np.uint8).reshape(B, 3, Ho, Wo) if colour else None, K=K)


# ---- the numpy restatement of the full scan -----------------------------------------------------------------------------------------

def _lerp(a, b, f):
    return a + f * (b - a)


def _tri(v, f):
    c00, c10, c01, c11 = _lerp(v[0], v[1], f[0]), _lerp(v[2], v[3], f[0]), _lerp(v[4], v[5], f[0]), _lerp(v[6], v[7], f[0])
    return _lerp(_lerp(c00, c10, f[1]), _lerp(c01, c11, f[1]), f[2])


def restate(vol, models, dirs, T_cv=None, near=NEAR, far=FAR, step=None, min_weight=1.0, colour=True):
    """csrc/tsdf_ray.h's ud_tsdf_ray with the full scan, for every pixel, in fp32 with every operation rounded separately.  dirs
    [B,3,Ho,Wo]; T_cv CAMERA TO VOLUME [1 or B,3,4] or None.  -> dict(depth, valid, points, normals, color_f32, color_u8) shaped as
    host_render's, and the scan's statistics: back (rays stopped by a back crossing), outside (rays with no sample in the grid),
    two_cells (hits whose two samples lie in different cells)"""
    B, (Nz, Ny, Nx) = vol["B"], vol["grid"]
    Ho, Wo = dirs.shape[2:]
    hw, n = Ho * Wo, Nz * Ny * Nx
    colour = colour and vol["color"] is not None
    step = F(vol["voxel"] if step is None else step)
    K = n_samples(near, far, step)
    near, vs, mw = F(near), F(vol["voxel"]), F(min_weight)
    d = np.asarray(dirs, F).reshape(B, 3, hw)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    o = np.broadcast_to(np.asarray(vol["origin"], F).reshape(-1, 3), (B, 3))
    T = None if T_cv is None else np.broadcast_to(np.asarray(T_cv, F).reshape(-1, 12), (B, 12))
    tsdf, weight = np.asarray(vol["tsdf"], F).reshape(B, n), np.asarray(vol["weight"], F).reshape(B, n)
    col = np.asarray(vol["color"], F).reshape(B, 3, n) if colour else None
    N = (Nx, Ny, Nz)

    def sample(t):
        p = [t * dx, t * dy, t * dz]
        if T is not None:
            p = [((T[:, 4 * r, None] * p[0] + T[:, 4 * r + 1, None] * p[1]) + T[:, 4 * r + 2, None] * p[2]) + T[:, 4 * r + 3, None] for r in range(3)]
        g = [(p[k] - o[:, k, None]) / vs - F(0.5) for k in range(3)]
        inside = np.ones((B, hw), bool)
        for k in range(3):
            inside &= (g[k] >= 0) & (g[k] <= F(N[k] - 1))
        lo, up, f = [], [], []
        for k in range(3):
            gs = np.where(inside, g[k], F(0))
            i = np.maximum(np.minimum(np.floor(gs).astype(np.int64), N[k] - 2), 0)
            lo.append(i)
            up.append(np.minimum(i + 1, N[k] - 1))
            f.append((gs - i.astype(F)).astype(F))
        idx = [(iz * Ny + iy) * Nx + ix for iz in (lo[2], up[2]) for iy in (lo[1], up[1]) for ix in (lo[0], up[0])]
        ok = inside.copy()
        for i in idx:
            ok &= np.take_along_axis(weight, i, 1) >= mw
        v = [np.take_along_axis(tsdf, i, 1) for i in idx]
        s = _tri(v, f)
        return ok & ~np.isnan(s), s, v, f, idx, inside

    def detail(v, f, idx):
        g = [_lerp(_lerp(v[1] - v[0], v[3] - v[2], f[1]), _lerp(v[5] - v[4], v[7] - v[6], f[1]), f[2]),
             _lerp(_lerp(v[2] - v[0], v[3] - v[1], f[0]), _lerp(v[6] - v[4], v[7] - v[5], f[0]), f[2]),
             _lerp(_lerp(v[4] - v[0], v[5] - v[1], f[0]), _lerp(v[6] - v[2], v[7] - v[3], f[0]), f[1])]
        c = [_tri([np.take_along_axis(col[:, k], i, 1) for i in idx], f) for k in range(3)] if colour else None
        return g, c

    zero = np.zeros((B, hw), F)
    have = done = hit = back = entered = two = np.zeros((B, hw), bool)
    sp, al, ts = zero, zero, zero
    G, C = [zero] * 3, [zero] * 3
    prev = prev_cell = None
    with np.errstate(all="ignore"):
        for k in range(K):
            t1 = near + F(k) * step
            valid, s, v, f, idx, inside = sample(t1)
            cur = detail(v, f, idx)
            entered = entered | inside
            both = valid & have & ~done
            now = both & ~(sp < 0) & (s < 0)
            if k > 0:
                t0 = near + F(k - 1) * step
                alk = sp / (sp - s)
                al = np.where(now, alk, al)
                ts = np.where(now, t0 + alk * (t1 - t0), ts)
                G = [np.where(now, prev[0][j] + alk * (cur[0][j] - prev[0][j]), G[j]) for j in range(3)]
                if colour:
                    C = [np.where(now, prev[1][j] + alk * (cur[1][j] - prev[1][j]), C[j]) for j in range(3)]
                two = two | (now & (idx[0] != prev_cell))
            stop = both & (sp < 0) & ~(s < 0)
            hit, back = hit | now, back | stop
            done = done | now | stop
            have, sp, prev, prev_cell = valid, s, cur, idx[0]
        x, y, z = ts * dx, ts * dy, ts * dz
        spherical = np.array([m == tc.SPHERICAL for m in models]).reshape(B, 1)
        dep = np.where(spherical, np.sqrt(x * x + y * y + z * z), z)
        valid = hit & (dep > 0)
        out = lambda a: np.where(valid, a, F(0)).astype(F)            # noqa: E731
        nx, ny, nz = G
        if T is not None:
            nx, ny, nz = ((T[:, c, None] * G[0] + T[:, 4 + c, None] * G[1]) + T[:, 8 + c, None] * G[2] for c in range(3))
        m = np.maximum(np.maximum(np.abs(nx), np.abs(ny)), np.abs(nz))
        good = np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz) & (m > 0)
        nx, ny, nz = nx / m, ny / m, nz / m
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / length, ny / length, nz / length
        flip = ((nx * x + ny * y) + nz * z) > 0
        nx, ny, nz = (np.where(flip, -c, c) for c in (nx, ny, nz))
        good = good & np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz) & valid
        normals = np.stack([np.where(good, c, F(0)).astype(F) for c in (nx, ny, nz)], axis=1)
        cf = np.stack([out(c) for c in C], axis=1) if colour else None
    shape = (B, 3, Ho, Wo)
    return dict(depth=out(dep).reshape(B, 1, Ho, Wo), valid=valid.reshape(B, 1, Ho, Wo), points=np.stack([out(x), out(y), out(z)], axis=1).reshape(shape),
                normals=normals.reshape(shape), color_f32=cf.reshape(shape) if colour else None,
                color_u8=tc.to_u8(cf).reshape(shape) if colour else None, K=K,
                back=int(back.sum()), outside=int((~entered).sum()), two_cells=int((two & valid).sum()))


def assert_same(got, want, what, names=("depth", "valid", "points", "normals", "color_f32", "color_u8")):
    """numpy dicts, bit for bit in every output"""
    for k in names:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if got[k] is not None and not same_bits(got[k], want[k]):
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
            diff = (a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1)
            raise AssertionError(f"{what}: {k} differs in {int(diff.sum())} of {diff.size} elements, first at {int(diff.nonzero()[0][0])}: "
                                 f"{a.reshape(-1)[diff][:4].tolist()} vs {b.reshape(-1)[diff][:4].tolist()}")


def assert_not_vacuous(what, r):
    """r: restate()'s result on a scene that is not tiny: the valid share strictly between 10 % and 90 %, a ray stopped by a back
    crossing, a ray that never enters the grid, a hit whose two samples lie in different cells"""
    share = float(r["valid"].mean())
    assert 0.1 < share < 0.9, (what, share)
    assert r["back"] >= 1 and r["outside"] >= 1 and r["two_cells"] >= 1, (what, r["back"], r["outside"], r["two_cells"])


# ---- the known answer ----------------------------------------------------------------------------------------------------------------

KNOWN_F = 32.0


def known_answer_volume(exe):
    """tsdf_common.known_answer_scene() integrated: tsdf = min(1, (2 - z) / 0.5) on a 4 x 4 x 12 grid of 0.25 voxels, centres x, y in
    +-0.125, +-0.375 and z = 0.625 .. 3.375, seen (weight 1) up to z = 2.375"""
    s = tc.known_answer_scene()
    r = tc.host_tsdf(exe, s)
    return dict(tsdf=r["tsdf"], weight=r["weight"], color=None, origin=np.array(s["origin"], F), voxel=s["voxel"], grid=s["grid"], B=1)


def known_rays(f=KNOWN_F):
    """the RAW Pinhole rays ((u - 8) / f, (v - 8) / f, 1) of the pixel centres of a 16 x 16 image"""
    c = (np.arange(16, dtype=F) + F(0.5) - F(8)) / F(f)
    r = np.ones((1, 3, 16, 16), F)
    r[0, 0] = c[None, :]
    r[0, 1] = c[:, None]
    return r


def check_known_answer(depth, valid, points, normals, f=KNOWN_F):
    """Every hit has depth == 2.0, normal == (0, 0, -1) and point z == 2.0 exactly.  The samples are z = 0.25, 0.5, ...; the block of
    valid cells spans |x|, |y| <= 0.375 and 0.625 <= z <= 2.375; a ray hits exactly when it is inside the block at z = 1.75 (tsdf 0.5) and
    z = 2.0 (0), and again at 2.25 (-0.5, the first negative sample): |x / z| * 2.25 <= 0.375.  Every ray that leaves the block before
    z = 2.25 must be invalid."""
    c = np.abs((np.arange(16, dtype=np.float64) + 0.5 - 8) / f)
    inside = (c * 2.25 <= 0.375)
    want = inside[:, None] & inside[None, :]
    assert want.mean() >= 0.25 and not want.all()
    assert np.array_equal(valid.reshape(16, 16), want)
    assert (depth.reshape(16, 16)[want] == F(2.0)).all() and (depth.reshape(16, 16)[~want] == 0).all()
    p, nr = points.reshape(3, 16, 16), normals.reshape(3, 16, 16)
    assert (p[2][want] == F(2.0)).all() and (p[0][want] == (F(2.0) * known_rays(f)[0, 0])[want]).all()
    assert (nr[0][want] == 0).all() and (nr[1][want] == 0).all() and (nr[2][want] == F(-1)).all() and (nr[:, ~want] == 0).all()


# ---- special values ------------------------------------------------------------------------------------------------------------------

def special_volume(v):
    """a volume of two images as one of three with NaN, +-inf and -0.0 spread over the distances and NaN, inf and negative values over
    the weights"""
    g = np.random.RandomState(9811)
    rep = lambda a: np.concatenate([a, a[:1]], axis=0)                # noqa: E731
    tsdf, weight = rep(np.array(v["tsdf"])), rep(np.array(v["weight"]))
    u = g.uniform(size=tsdf.shape)
    tsdf[u < 0.02] = np.nan
    tsdf[(u >= 0.02) & (u < 0.04)] = np.inf
    tsdf[(u >= 0.04) & (u < 0.06)] = -np.inf
    tsdf[(u >= 0.06) & (u < 0.09) & (tsdf >= 0) & (tsdf < 0.2)] = -0.0
    u = g.uniform(size=tsdf.shape)
    weight[u < 0.02] = np.nan
    weight[(u >= 0.02) & (u < 0.04)] = np.inf
    weight[(u >= 0.04) & (u < 0.06)] = -1.0
    return dict(v, tsdf=tsdf, weight=weight, color=rep(np.array(v["color"])), B=3)


def special_inputs():
    """for three images: rays with NaN, zero and infinite components; image 1's transform with a NaN in one entry, image 2's mirrored
    (x -> -x) -> (T_cv [3,3,4] CAMERA TO VOLUME, rays [3,3,Ho,Wo], params, models).  The tests make image 0 a singular Pinhole (fx = 0)
    in the camera form."""
    T = invert(transforms(True, B=3))
    T[1, 1, 2] = np.nan
    T[2, :, 0] = -T[2, :, 0]
    models = (tc.PINHOLE, tc.EUCM, tc.MEI)
    Ho, Wo = SIZE
    rays = np.zeros((3, 3, Ho, Wo), F)
    rays[:, 2] = 1
    rays[:, 0] = ((np.arange(Wo, dtype=F) + F(0.5) - F(Wo / 2)) / F(14))[None, None, :]
    rays[:, 1] = ((np.arange(Ho, dtype=F) + F(0.5) - F(Ho / 2)) / F(14))[None, :, None]
    rays[:, 0, ::3, ::4] = np.nan
    rays[:, 1, 1::3, 1::4] = np.inf
    rays[:, 2, 2::3, 2::4] = -np.inf
    rays[:, 0, :, 9] = 0.0
    rays[:, :, 5, 5] = 0.0
    return T, rays, params_for(models, SIZE), models


def special_case(exe):
    """(special_volume of the base volume,) + special_inputs()"""
    return (special_volume(volume(exe, colour=True)),) + special_inputs()


def check_special(r):
    """finite where valid, exactly 0 where not"""
    v = r["valid"]
    v3 = np.broadcast_to(v, r["points"].shape)
    assert np.isfinite(r["depth"][v]).all() and (r["depth"][v] > 0).all() and np.isfinite(r["points"][v3]).all() and np.isfinite(r["normals"]).all()
    for k in ("depth", "points", "normals", "color_f32", "color_u8"):
        if r[k] is not None:
            a = r[k]
            assert (a[~np.broadcast_to(v, a.shape)] == 0).all() and not np.signbit(a[~np.broadcast_to(v, a.shape)].astype(F)).any(), k
    if r["color_f32"] is not None:
        assert np.isfinite(r["color_f32"]).all()
