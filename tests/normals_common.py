"""What the surface-normal tests share (not a test module): the numpy fp32 RESTATEMENT of the definition of a normal and of the normal
metrics (include/unidepth_hip.h, UdNormals / UdEvalNormals) -- the oracle; the reference has no normals code --, the seeded scene, the
special values and the call of the host program tests/normals_host/normals_host.cpp.

Every numpy operation below works on float32 arrays and rounds once, in the order the definition writes them; numpy never fuses a multiply
with an add."""
import functools
import math

import numpy as np

import host_program
import warp_common as wc
from host_program import ROOT, f32_bits, same_bits  # noqa: F401  (the tests reach them through this module)

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = wc.PINHOLE, wc.EUCM, wc.SPHERICAL, wc.OPENCV, wc.FISHEYE624, wc.MEI
CLOSED = wc.CLOSED
H0, W0, B0 = 37, 53, 6
MODELS = (PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI)          # the scene's batch holds all six
EDGE_RTOL = 0.05
THRESHOLDS = (11.25, 22.5, 30.0)
PRED_NOISE = 0.02                                                     # see pred_depth()
# the conditions of the scene, asserted per image so that nothing passes by marking everything invalid
VALID_SHARE = (0.5, 0.95)
ONE_SIDED_MIN = 0.2
EDGE_REJECTED_MIN = 0.02
F32 = np.float32


def rows(models):
    return wc.rows(models, wc.DST_ROWS)


# ---- the restatement of a normal ---------------------------------------------------------------------------------------------------

def _shift(a, oy, ox, fill):
    """out[..., y, x] = a[..., y + oy, x + ox], `fill` outside the image"""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    ys, yd = (slice(oy, H), slice(0, H - oy)) if oy >= 0 else (slice(0, H + oy), slice(-oy, H))
    xs, xd = (slice(ox, W), slice(0, W - ox)) if ox >= 0 else (slice(0, W + ox), slice(-ox, W))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def restate_normals(points, mask=None, depth=None, edge_rtol=None):
    """points fp32 [B,3,H,W]; mask [B or 1,H,W] / [.,1,H,W] or None; depth [B,H,W] / [B,1,H,W] or None
    -> dict(normals fp32 [B,3,H,W], valid bool [B,H,W], rgb uint8 [B,3,H,W], one_sided, edge_rejected, flipped bool [B,H,W])"""
    P = np.ascontiguousarray(points, F32)
    Bn, _, H, W = P.shape
    ok = np.isfinite(P).all(axis=1)
    if mask is not None:
        ok = ok & (np.broadcast_to(np.asarray(mask).reshape(-1, H, W), (Bn, H, W)) != 0)
    d = P[:, 2] if depth is None else np.ascontiguousarray(depth, F32).reshape(Bn, H, W)
    use, pts, lost = {}, {}, np.zeros((Bn, H, W), bool)
    with np.errstate(all="ignore"):
        for name, (oy, ox) in dict(L=(0, -1), R=(0, 1), U=(-1, 0), D=(1, 0)).items():
            u = _shift(ok, oy, ox, False)                                # inside the image and ok
            if edge_rtol is not None:
                dq = _shift(d, oy, ox, F32(0))
                lo = np.where(dq < d, dq, d)
                e = np.abs(d - dq) <= F32(edge_rtol) * lo                # false for a NaN
                lost |= ok & u & ~e
                u = u & e
            use[name], pts[name] = u, _shift(P, oy, ox, F32(0))
        dx = np.where(use["R"][:, None], pts["R"], P) - np.where(use["L"][:, None], pts["L"], P)
        dy = np.where(use["D"][:, None], pts["D"], P) - np.where(use["U"][:, None], pts["U"], P)
        nx = dy[:, 1] * dx[:, 2] - dy[:, 2] * dx[:, 1]
        ny = dy[:, 2] * dx[:, 0] - dy[:, 0] * dx[:, 2]
        nz = dy[:, 0] * dx[:, 1] - dy[:, 1] * dx[:, 0]
        m = np.maximum(np.maximum(np.abs(nx), np.abs(ny)), np.abs(nz))   # a NaN passes through
        valid = ok & (use["L"] | use["R"]) & (use["U"] | use["D"]) & (m > 0) & np.isfinite(m)
        nx, ny, nz = nx / m, ny / m, nz / m
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        s = (nx * P[:, 0] + ny * P[:, 1]) + nz * P[:, 2]
        flip = s > 0
        n = np.stack([np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)], axis=1)
        n = np.where(valid[:, None], n, F32(0)).astype(F32)
        q = np.floor((n + F32(1)) * F32(127.5) + F32(0.5))
        rgb = np.where(valid[:, None], np.clip(q, 0, 255), 0).astype(np.uint8)
    assert n.dtype == F32 and dx.dtype == F32 and m.dtype == F32 and s.dtype == F32
    one_sided = valid & ((use["L"] ^ use["R"]) | (use["U"] ^ use["D"]))
    return dict(normals=n, valid=valid, rgb=rgb, one_sided=one_sided, edge_rejected=lost, flipped=valid & flip)


def check_conditions(r, edge):
    """the scene's conditions on a restatement's result, per image"""
    for b in range(r["valid"].shape[0]):
        v = r["valid"][b]
        share = v.mean()
        assert VALID_SHARE[0] <= share <= VALID_SHARE[1], (b, share)
        assert r["one_sided"][b].sum() >= ONE_SIDED_MIN * v.sum(), (b, r["one_sided"][b].sum(), v.sum())
        if edge:
            assert r["edge_rejected"][b].mean() >= EDGE_REJECTED_MIN, (b, r["edge_rejected"][b].mean())


# ---- the restatement of the metrics --------------------------------------------------------------------------------------------------

def cos_of(t):
    """the fp32 rounding of the float64 cosine of a threshold in degrees"""
    return F32(math.cos(math.radians(t)))


def restate_cos(gt, pred, mask=None):
    """-> (c fp32 [B,H,W], use bool [B,H,W]): the clamped cosine and the pixels that count"""
    g, p = np.ascontiguousarray(gt, F32), np.ascontiguousarray(pred, F32)
    Bn, _, H, W = g.shape
    use = np.isfinite(g).all(axis=1) & np.isfinite(p).all(axis=1)
    if mask is not None:
        use = use & (np.broadcast_to(np.asarray(mask).reshape(-1, H, W), (Bn, H, W)) != 0)
    with np.errstate(all="ignore"):
        lg = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        lp = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        use = use & (lg > 0) & np.isfinite(lg) & (lp > 0) & np.isfinite(lp)
        c = ((g[:, 0] * p[:, 0] + g[:, 1] * p[:, 1]) + g[:, 2] * p[:, 2]) / (lg * lp)
        use = use & ~np.isnan(c)
        c = np.where(c < F32(-1), F32(-1), np.where(c > F32(1), F32(1), c))
    assert c.dtype == F32
    return c, use


def restate_eval(gt, pred, mask=None, thresholds=THRESHOLDS):
    """-> dict(mean, median, rmse float64 [B] (degrees, from the float64 acos of the fp32 cosine), a_<t> fp32 [B], n_<t> int [B] (the
    counts), count int64 [B], error float64 [B,H,W] (NaN where dropped))"""
    c, use = restate_cos(gt, pred, mask)
    Bn = c.shape[0]
    err = np.where(use, np.degrees(np.arccos(np.where(use, c, F32(0)).astype(np.float64))), np.nan)
    out = {k: np.full(Bn, np.nan) for k in ("mean", "median", "rmse")}
    out["count"] = use.reshape(Bn, -1).sum(axis=1).astype(np.int64)
    for t in thresholds:
        out[f"a_{t}"], out[f"n_{t}"] = np.full(Bn, np.nan, F32), np.zeros(Bn, np.int64)
    for b in range(Bn):
        n = int(out["count"][b])
        if n == 0:
            continue
        e = np.sort(err[b][use[b]])
        out["mean"][b], out["rmse"][b], out["median"][b] = e.mean(), math.sqrt((e * e).mean()), e[(n - 1) // 2]
        for t in thresholds:
            k = int((c[b][use[b]] > cos_of(t)).sum())
            out[f"n_{t}"][b], out[f"a_{t}"][b] = k, F32(k) / F32(n)
    out["error"] = err
    return out


def plain_eval(gt, pred, mask=None, thresholds=THRESHOLDS):
    """the textbook float64 formulation: arccos of the normalised dot product, np.sort for the lower median, `<` for the shares"""
    g, p = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    Bn, _, H, W = g.shape
    with np.errstate(all="ignore"):
        lg, lp = np.linalg.norm(g, axis=1), np.linalg.norm(p, axis=1)
        use = np.isfinite(g).all(axis=1) & np.isfinite(p).all(axis=1) & (lg > 0) & (lp > 0)
        if mask is not None:
            use = use & (np.broadcast_to(np.asarray(mask).reshape(-1, H, W), (Bn, H, W)) != 0)
        e = np.degrees(np.arccos(np.clip((g * p).sum(axis=1) / (lg * lp), -1.0, 1.0)))
    out = dict(count=use.reshape(Bn, -1).sum(axis=1), mean=np.full(Bn, np.nan), median=np.full(Bn, np.nan), rmse=np.full(Bn, np.nan))
    for t in thresholds:
        out[f"n_{t}"] = np.zeros(Bn, np.int64)
    for b in range(Bn):
        v = np.sort(e[b][use[b]])
        if v.size:
            out["mean"][b], out["rmse"][b], out["median"][b] = v.mean(), math.sqrt((v * v).mean()), v[(v.size - 1) // 2]
            for t in thresholds:
                out[f"n_{t}"][b] = int((v < t).sum())
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene(H=H0, W=W0, noise_seed=0, noise=0.002, Bn=B0):
    """per image: depth = 2 + 0.6 x / W + 0.9 y / H + noise N(0, 1), the central box (rows H/4..3H/4, columns W/3..2W/3) times 0.6 -- a
    depth step --, 2 % NaN and 1 % zeros, and a mask with 10 % holes.  The holes and the mask depend on the size alone, the noise on
    noise_seed.  -> (depth fp32 [B,1,H,W], mask uint8 [B,1,H,W]), read-only"""
    g = np.random.RandomState(9400 + 131 * H + W)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 2.0 + 0.6 * x / W + 0.9 * y / H + noise * np.random.RandomState(9500 + noise_seed).normal(size=(Bn, 1, H, W))
    depth[:, :, H // 4:3 * H // 4, W // 3:2 * W // 3] *= 0.6
    depth = depth.astype(F32)
    hole = g.uniform(size=depth.shape)
    depth[hole < 0.02] = np.nan
    depth[(hole >= 0.02) & (hole < 0.03)] = 0.0
    mask = (g.uniform(size=depth.shape) >= 0.10).astype(np.uint8)
    depth.setflags(write=False)
    mask.setflags(write=False)
    return depth, mask


def pred_depth(H=H0, W=W0):
    """the same scene with another noise seed.  The amplitude PRED_NOISE: a pixel is 2 / 50 = 0.04 wide at the scene's depth and focal
    length, so a depth noise of sigma tilts a central difference by about atan(sqrt(2) sigma / 0.08) and a one-sided one by twice that
    slope; 0.02 gives about 19 and 35 degrees -- errors spread over all three thresholds.  test_normals_cpu.py asserts on the restatement
    alone that every share of every image lies inside (0.05, 0.95)."""
    return scene(H, W, noise_seed=1, noise=PRED_NOISE)[0]


def special_depth():
    """the scene's depth with the special values at the head of the first two rows of every image, as warp_common.special_case lays
    them out: 0, negative, NaN, +inf / +inf, -inf, -0.0, 1e-30"""
    depth = np.array(scene()[0])
    depth[:, 0, 0, 0:4] = [0.0, -3.0, np.nan, np.inf]
    depth[:, 0, 1, 0:4] = [np.inf, -np.inf, -0.0, 1e-30]
    return depth


def special_points():
    """point maps [5,3,9,11] (x, y, 2 + 0.1 x) with: image 0 scaled to 1e30 (the cross product overflows: invalid everywhere); image 1
    with neighbours 1e-30 apart (the products underflow, m = 0: invalid everywhere); image 2 with coincident neighbours in a block (the
    differences vanish there) and a NaN, an inf and a -inf coordinate; image 3 with x negated and image 4 with y negated (mirrored clouds)"""
    H, W = 9, 11
    y, x = np.mgrid[0:H, 0:W].astype(F32)
    base = np.stack([x - 5, y - 4, 2 + F32(0.1) * x]).astype(F32)
    p = np.stack([base * F32(1e30), base * F32(1e-30), base, base * np.array([-1, 1, 1], F32)[:, None, None],
                  base * np.array([1, -1, 1], F32)[:, None, None]]).astype(F32)
    p[2, :, 2:5, 3:7] = p[2, :, 2:3, 3:4]
    p[2, 0, 6, 2], p[2, 1, 6, 6], p[2, 2, 7, 8] = np.nan, np.inf, -np.inf
    return p


def known_answers():
    """[(points [1,3,6,7], the normal every pixel must have)]: P = (x, y, 2) -> (0, 0, -1); P = (x, y, x + 8) -> (1, 0, -1) / sqrt 2"""
    y, x = np.mgrid[0:6, 0:7].astype(F32)
    r = F32(1) / np.sqrt(F32(2))
    return [(np.stack([x, y, np.full_like(x, 2)])[None], (F32(0), F32(0), F32(-1))),
            (np.stack([x, y, x + F32(8)])[None], (r, F32(0), -r))]


def check_known_answer(run):
    """run(points) -> (normals, valid) as numpy"""
    for pts, want in known_answers():
        n, valid = run(pts)
        assert valid.all()
        for k in range(3):
            assert (n[:, k] == want[k]).all(), (k, want, n[:, k])


# ---- the host program ----------------------------------------------------------------------------------------------------------------

def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "normals_host")


def host_normals(exe, *, points=None, depth=None, params=None, models=None, mask=None, edge_rtol=None):
    """tests/normals_host on numpy inputs: the points form (points [, depth]) or the depth form (depth, params, models)
    -> dict(normals [B,3,H,W], valid bool [B,H,W], rgb [B,3,H,W], points [B,3,H,W] in the depth form)"""
    form = int(points is None)
    geo = depth if form else points
    Bn, (H, W) = geo.shape[0], geo.shape[-2:]
    n = H * W
    blobs = []
    if form == 0:
        blobs.append(np.ascontiguousarray(points, F32).tobytes())
    if depth is not None:
        blobs.append(np.ascontiguousarray(depth, F32).tobytes())
    if form:
        blobs.append(np.ascontiguousarray(params, F32).tobytes())
    mb = 0
    if mask is not None:
        m = np.ascontiguousarray(mask, np.uint8).reshape(-1, H, W)
        mb = m.shape[0]
        blobs.append(m.tobytes())
    args = [form, Bn, H, W, mb, int(depth is not None), int(edge_rtol is not None), f32_bits(edge_rtol or 0.0)]
    args += list(models) if models is not None else [0] * Bn
    part = host_program.run(exe, args, blobs, [Bn * 3 * n * 4, Bn * n, Bn * 3 * n, Bn * 3 * n * 4 if form else 0])
    return dict(normals=np.frombuffer(part[0], F32).reshape(Bn, 3, H, W), valid=np.frombuffer(part[1], np.uint8).reshape(Bn, H, W).astype(bool),
                rgb=np.frombuffer(part[2], np.uint8).reshape(Bn, 3, H, W),
                points=np.frombuffer(part[3], F32).reshape(Bn, 3, H, W) if form else None)


def assert_same(got, want, what=""):
    """normals (as integers: the sign of a zero counts), valid and rgb, every element"""
    for k in ("normals", "valid", "rgb"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if k == "normals":
            a, b = a.astype(F32).view(np.uint32), b.astype(F32).view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what}: {k} differs in {len(bad)} of {a.size} elements, first at {tuple(bad[0])}: "
                                 f"{got[k][tuple(bad[0])]!r} vs {want[k][tuple(bad[0])]!r}")
