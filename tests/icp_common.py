"""What the ICP tests share (not a test module): the numpy restatement of csrc/icp_point.h -- ud_icp_row in fp32, the system in fp64 and
ud_icp_solve operation by operation in fp64 -- the two scenes with known answers (the corner of three planes, the smooth surface), the
call of the host program tests/icp_host/icp_host.cpp, and the errors of a pose.  The restatement computes the Pinhole models itself (no
libm function beyond the square root); for the other camera models it takes the frame's points and the image coordinates from the host
program's chain of the unchanged per-point functions, whose arithmetic the tests of those functions cover.  The oracle of the GPU tests
is unidepth_amd.icp's composition of the merged calls, never the fused kernels."""
import functools
import struct

import numpy as np

import host_program
import tsdf_common as tc
from host_program import ROOT, bits, f32_bits, same_bits  # noqa: F401  (the tests reach them through this module)

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = 1, 2, 3, 4, 5, 6
MODELS = (PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI)
CLOSED = (PINHOLE, EUCM, SPHERICAL, MEI)
NAMES = tc.NAMES
F = np.float32
FLT_MAX = F(3.402823466e38)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]
SPAN = 256 * 256                       # the grid-stride span of icp_rows_kernel: nblk = min(ceil(n / 256), 256) workgroups of 256 threads


def f64_bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


# ---- poses -------------------------------------------------------------------------------------------------------------------------

def cayley(omega):
    """R = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = omega / 2, in fp64"""
    a = np.asarray(omega, np.float64) / 2
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return ((1 - a @ a) * np.eye(3) + 2 * np.outer(a, a) + 2 * K) / (1 + a @ a)


def pose(omega, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = cayley(omega), t
    return T


def pose_errors(T, truth):
    """(rotation error in degrees, translation error) of a [3,4] / [4,4] estimate against the truth; the angle of D = R^T R* as
    atan2(|vee(D - D^T)| / 2, (tr D - 1) / 2), which resolves angles far below the 2e-2 degrees at which the arc cosine of the trace stops"""
    T, truth = np.asarray(T, np.float64), np.asarray(truth, np.float64)
    D = T[:3, :3].T @ truth[:3, :3]
    s = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(s), (np.trace(D) - 1) / 2))), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


# ---- the restatement of ud_icp_row -------------------------------------------------------------------------------------------------

def pinhole_points(depth, row):
    """ud_cam_unproject_closed(PINHOLE, UD_UNPROJ_DEPTH) on the identity grid at pixel centres: depth fp32 [H,W] -> fp32 [3,H,W]"""
    H, W = depth.shape
    fx, fy, cx, cy = (F(v) for v in row[:4])
    u = (np.arange(W, dtype=F) + F(0.5))[None, :].repeat(H, 0)
    v = (np.arange(H, dtype=F) + F(0.5))[:, None].repeat(W, 1)
    with np.errstate(all="ignore"):
        x, y = (u - cx) / fx, (v - cy) / fy
        z = ((F(0) * (fx + fy + cx + cy) + F(0) * u) + F(0) * v) + F(1)
        zc = np.where(z < F(1e-4), F(1e-4), z)
        dc = np.where(depth < F(0), F(0), depth)
        return np.stack([x / zc * dc, y / zc * dc, z / zc * dc]).astype(F)


def move(T, P):
    """ud_cam_move: T fp32 [3,4], P fp32 [3,...]"""
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * P[0] + T[r, 1] * P[1]) + T[r, 2] * P[2]) + T[r, 3] for r in range(3)]).astype(F)


def pinhole_project(row, Q):
    fx, fy, cx, cy = (F(v) for v in row[:4])
    with np.errstate(all="ignore"):
        zc = np.where(Q[2] < F(0.01), F(0.01), Q[2])
        return ((fx * Q[0] + cx * Q[2]) / zc).astype(F), ((fy * Q[1] + cy * Q[2]) / zc).astype(F)


def inside(model, u, v, z, H, W):
    """ud_cam_inside, the comparisons taken literally"""
    with np.errstate(all="ignore"):
        w, h = F(W), F(H)
        if model == PINHOLE:
            return (u >= 0) & (u < w) & (v >= 0) & (v < h)
        out = (u < 0) | (u > w) | (v < 0) | (v > h)
        if model == EUCM:
            out = out | (z < 0)
        return ~out


def cam_depth(model, Q):
    with np.errstate(all="ignore"):
        return np.sqrt(Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2]).astype(F) if model == SPHERICAL else Q[2]


def _nearest(coord, size):
    """ud_rm_axis in nearest mode, zeros padding: the clamp that sends a NaN to its lower end, then round half to even"""
    with np.errstate(all="ignore"):
        p = coord - F(0.5)
        lo, hi = F(-2.0), F(size + 1)
        q = np.where(p >= lo, np.where(p <= hi, p, hi), lo)
        return np.rint(q).astype(np.int64)


def finite(x):
    with np.errstate(all="ignore"):
        return np.abs(x) <= FLT_MAX


def restate_rows(P, live, T, model, row_model, mp, mn, mv, dist_tol, uv=None, normals=None, cos_tol=None, weights=None):
    """ud_icp_row for one image.  P fp32 [3,H,W] the frame's points, live bool [H,W] (depth > 0 or the points finite, and the mask), T fp32
    [3,4], the model camera's tag and row, the model maps [3,Hm,Wm] x 2 and valid [Hm,Wm].  uv: the image coordinates for a model camera
    that is not a Pinhole.  -> matched bool [H,W], residual fp32 [H,W], rows fp32 [6,H,W] (0 where not matched), w fp32 [H,W]"""
    Hm, Wm = mv.shape
    shape = P.shape[1:]
    w = np.ones(shape, F) if weights is None else weights.astype(F)
    with np.errstate(all="ignore"):
        live = live & (w > 0) & finite(w)
        Q = move(T, P)
        u, v = pinhole_project(row_model, Q) if uv is None else (uv[0], uv[1])
        usable = inside(model, u, v, Q[2], Hm, Wm) & (cam_depth(model, Q) > 0) & finite(u) & finite(v)
        x, y = _nearest(u, Wm), _nearest(v, Hm)
        in_range = (x >= 0) & (x < Wm) & (y >= 0) & (y < Hm)
        off = np.where(in_range, y * Wm + x, 0)
        tap = in_range & (mv.reshape(-1)[off] != 0)
        m = np.where(tap, mp.reshape(3, -1)[:, off], F(0)).astype(F)
        n = np.where(tap, mn.reshape(3, -1)[:, off], F(0)).astype(F)
        model_ok = tap & (u >= 0) & (u <= F(Wm)) & (v >= 0) & (v <= F(Hm))
        e = m - Q
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
        c = [Q[1] * n[2] - Q[2] * n[1], Q[2] * n[0] - Q[0] * n[2], Q[0] * n[1] - Q[1] * n[0]]
        g = np.stack(c + [n[0], n[1], n[2]]).astype(F)
        tol = F(dist_tol)
        tol2 = tol * tol
        matched = live & usable & model_ok & (n != 0).any(axis=0) & (d2 <= tol2)
        if normals is not None and cos_tol is not None:
            f = normals.astype(F)
            rot = [(T[k, 0] * f[0] + T[k, 1] * f[1]) + T[k, 2] * f[2] for k in range(3)]
            matched = matched & ((rot[0] * n[0] + rot[1] * n[1]) + rot[2] * n[2] >= F(cos_tol))
        matched = matched & finite(r) & finite(g).all(axis=0)
    return matched, np.where(matched, r, F(0)).astype(F), np.where(matched, g, F(0)).astype(F), w


def terms(matched, r, g, w):
    """the 30 columns of fp64 terms of the matched pixels in pixel order, [count, 30]: (w g_i) g_j for i <= j, (w g_i) r, (w r) r, w, 1"""
    k = matched.reshape(-1)
    gd, rd, wd = g.reshape(6, -1)[:, k].astype(np.float64), r.reshape(-1)[k].astype(np.float64), w.reshape(-1)[k].astype(np.float64)
    gw = wd * gd
    cols = [gw[i] * gd[j] for i, j in TRI] + [gw[i] * rd for i in range(6)] + [(wd * rd) * rd, wd, np.ones_like(wd)]
    return np.stack(cols, axis=1) if len(wd) else np.zeros((0, 30))


def system(t, serial):
    """fp64 [32] from the terms: serial=True in pixel order, one running sum per slot starting at 0 (the host program's order, bit for
    bit); else numpy's own sum"""
    S = np.zeros(32)
    if len(t):
        S[:30] = np.cumsum(np.concatenate([np.zeros((1, 30)), t]), axis=0)[-1] if serial else t.sum(axis=0)
    return S


def system_bound(t):
    """|dS| <= 2 n 2^-53 sum |t| per slot: any two orders of summing n terms differ by at most that (each within (n - 1) u sum |t| of the
    exact sum, u = 2^-53, to first order; the factor 2 n in place of 2 (n - 1) covers the higher orders for n u << 1)"""
    S = np.zeros(32)
    S[:30] = 2 * len(t) * 2.0 ** -53 * np.abs(t).sum(axis=0)
    return S


# ---- the restatement of ud_icp_solve -----------------------------------------------------------------------------------------------

def solve(S, T, damping=0.0, min_count=6):
    """ud_icp_solve for one image, operation by operation in fp64 (numpy scalars): S fp64 [32], T fp32 [3,4] -> (T_new fp32 [3,4], x fp64
    [6], status)"""
    D = np.float64
    S = np.asarray(S, D)
    zero_x = np.zeros(6)
    with np.errstate(all="ignore"):
        A = np.zeros((6, 6))
        for k, (i, j) in enumerate(TRI):
            A[i, j] = A[j, i] = S[k]
        for i in range(6):
            A[i, i] = A[i, i] + D(damping)

        def dot(ts):
            s = None
            for t in ts:
                s = t if s is None else s + t
            return s

        L, d = np.zeros((6, 6)), np.zeros(6)
        for j in range(6):
            d[j] = A[j, j] if j == 0 else A[j, j] - dot((L[j, c] * L[j, c]) * d[c] for c in range(j))
            if not d[j] > 0:
                return T.copy(), zero_x, 0
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] if j == 0 else A[i, j] - dot((L[i, c] * L[j, c]) * d[c] for c in range(j))) / d[j]
        y = np.zeros(6)
        for i in range(6):
            y[i] = S[21 + i] if i == 0 else S[21 + i] - dot(L[i, c] * y[c] for c in range(i))
        z = y / d
        x = np.zeros(6)
        for i in range(5, -1, -1):
            x[i] = z[i] if i == 5 else z[i] - dot(L[c, i] * x[c] for c in range(i + 1, 6))
        if not (S[29] >= D(min_count) and np.isfinite(x).all()):
            return T.copy(), zero_x, 0
        a0, a1, a2 = x[0] * D(0.5), x[1] * D(0.5), x[2] * D(0.5)
        aa = (a0 * a0 + a1 * a1) + a2 * a2
        den, kk, t0, t1, t2 = D(1) + aa, D(1) - aa, D(2) * a0, D(2) * a1, D(2) * a2
        R = np.array([[(kk + t0 * a0) / den, (t0 * a1 - t2) / den, (t0 * a2 + t1) / den],
                      [(t1 * a0 + t2) / den, (kk + t1 * a1) / den, (t1 * a2 - t0) / den],
                      [(t2 * a0 - t1) / den, (t2 * a1 + t0) / den, (kk + t2 * a2) / den]])
        O = T.astype(D)
        N = np.zeros((3, 4))
        for i in range(3):
            for j in range(4):
                N[i, j] = (R[i, 0] * O[0, j] + R[i, 1] * O[1, j]) + R[i, 2] * O[2, j]
            N[i, 3] = N[i, 3] + x[3 + i]
        return N.astype(F), x, 1


def track(P, live, T, model, row_model, mp, mn, mv, dist_tol, iters, damping=0.0, min_count=6, **kw):
    """the restated loop for one image, sums in pixel order -> T fp32 [3,4], and per step (system, x, status, T, matched share of live)"""
    T = np.array(T, F)
    steps = []
    for _ in range(iters):
        matched, r, g, w = restate_rows(P, live, T, model, row_model, mp, mn, mv, dist_tol, **kw)
        S = system(terms(matched, r, g, w), serial=True)
        T, x, status = solve(S, T, damping, min_count)
        steps.append(dict(S=S, x=x, status=status, T=T.copy(), share=matched.sum() / max(live.sum(), 1), matched=int(matched.sum())))
    return T, steps


# ---- the scenes --------------------------------------------------------------------------------------------------------------------

def pinhole_row(H, W, f):
    return tc.row_for(PINHOLE, H, W, f)


def _grid(H, W, f):
    x = (np.arange(W) + 0.5 - W / 2) / f
    y = (np.arange(H) + 0.5 - H / 2) / f
    return np.meshgrid(x, y)


PLANES = ((0, -1.2), (1, 1.0), (2, 3.0))               # axis, value: x = -1.2, y = 1.0, z = 3.0 in the world
POSE_A = pose((0.05, -0.1, 0.0), (0, 0, 0))
POSE_B = pose((0.03, -0.04, 0.02), (0.05, -0.03, 0.04)) @ POSE_A
CORNER_TRUTH = POSE_A @ np.linalg.inv(POSE_B)          # frame (B) camera -> model (A) camera: 3.08 degrees, 0.0707
CORNER_TOL = 0.2
CORNER_SIZES = {"48x64": ((48, 64, 40.0), None), "24x32": ((24, 32, 20.0), None), "37x53": ((37, 53, 33.0), None),
                "29x41_37x53": ((29, 41, 25.0), (37, 53, 33.0))}          # frame (H, W, f), model (H, W, f) or the same
CORNER_BARS = (0.25, 0.01)                             # degrees, translation, after 8 iterations
# what the restated loop reaches after 8 iterations (rotation error in degrees, translation error), rounded up in the last digit
CORNER_MEASURED = {"48x64": (0.0221, 1.9e-4), "24x32": (0.0846, 5.1e-3), "37x53": (0.0659, 2.7e-3), "29x41_37x53": (0.1261, 5.1e-3)}
# the smooth scene's floor with fp32 rows: the largest error of the restated loop over iterations 3 .. 6 and the three sizes (the pose
# jitters there from step to step by the rounding of T to fp32); the bar after 6 iterations is 8 times that
SMOOTH_FLOOR = (5.6e-5, 8.2e-7)


def corner_view(P, H, W, f):
    """the corner seen through a pinhole at the world->camera pose P: depth [H,W], points [3,H,W], normals [3,H,W] (the plane's normal
    turned towards the camera), all fp64, analytic: the nearest positive ray-plane intersection"""
    R, t = P[:3, :3], P[:3, 3]
    c = -R.T @ t
    gx, gy = _grid(H, W, f)
    dc = np.stack([gx, gy, np.ones_like(gx)])
    dw = np.einsum("ij,jhw->ihw", R.T, dc)
    best, which = np.full((H, W), np.inf), np.zeros((H, W), int)
    for k, (axis, value) in enumerate(PLANES):
        with np.errstate(all="ignore"):
            s = (value - c[axis]) / dw[axis]
        hit = (s > 0) & (s < best)
        best, which = np.where(hit, s, best), np.where(hit, k, which)
    pts = dc * best
    nrm = np.zeros((3, H, W))
    for k, (axis, _) in enumerate(PLANES):
        n = R[:, axis]
        sign = np.where((n[:, None, None] * pts).sum(0) > 0, -1.0, 1.0)
        nrm = np.where(which == k, n[:, None, None] * sign, nrm)
    return best, pts, nrm


@functools.lru_cache(maxsize=None)
def corner(name):
    (H, W, f), model = CORNER_SIZES[name]
    Hm, Wm, fm = model or (H, W, f)
    depth = corner_view(POSE_B, H, W, f)[0].astype(F)
    _, mp, mn = corner_view(POSE_A, Hm, Wm, fm)
    return dict(name=name, H=H, W=W, Hm=Hm, Wm=Wm, depth=depth, row=pinhole_row(H, W, f), row_model=pinhole_row(Hm, Wm, fm), mp=mp.astype(F),
                mn=mn.astype(F), mv=np.ones((Hm, Wm), np.uint8), T0=np.eye(4, dtype=F)[:3], truth=CORNER_TRUTH, dist_tol=CORNER_TOL)


SMOOTH_SIZES = {"48x64": (48, 64, 60.0), "24x32": (24, 32, 30.0), "37x53": (37, 53, 50.0)}
SMOOTH_START = pose((0.02, -0.03, 0.015), (0.03, -0.02, 0.04))
SMOOTH_TOL = 0.1


@functools.lru_cache(maxsize=None)
def smooth(name):
    H, W, f = SMOOTH_SIZES[name]
    gx, gy = _grid(H, W, f)
    depth = (2 + 0.4 * np.sin(2 * gx) + 0.3 * np.cos(2.5 * gy) + 0.2 * gx * gy).astype(F)
    row = pinhole_row(H, W, f)
    mp = pinhole_points(depth, row)                                   # the same view: gt_points' restatement
    P = mp.astype(np.float64)
    du, dv = np.zeros_like(P), np.zeros_like(P)
    du[:, :, 1:-1], dv[:, 1:-1, :] = P[:, :, 2:] - P[:, :, :-2], P[:, 2:, :] - P[:, :-2, :]
    n = np.cross(du, dv, axis=0)
    with np.errstate(all="ignore"):
        n = n / np.linalg.norm(n, axis=0)
    n = np.where((n * P).sum(0) > 0, -n, n)
    mv = np.zeros((H, W), np.uint8)
    mv[1:-1, 1:-1] = 1
    mn = np.where(mv.astype(bool), n, 0).astype(F)
    return dict(name=name, H=H, W=W, Hm=H, Wm=W, depth=depth, row=row, row_model=row, mp=mp, mn=mn, mv=mv, T0=SMOOTH_START[:3].astype(F),
                truth=np.eye(4), dist_tol=SMOOTH_TOL)


def restated_track(s, iters, **kw):
    """the restated loop on a scene from its start"""
    P = pinhole_points(s["depth"], s["row"])
    return track(P, s["depth"] > 0, s["T0"], PINHOLE, s["row_model"], s["mp"], s["mn"], s["mv"], s["dist_tol"], iters, **kw)


# ---- the host program --------------------------------------------------------------------------------------------------------------

def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "icp_host")


def host_run(exe, *, depth=None, points=None, params=None, models_frame=None, mp, mn, mv, params_model, models_model, T, dist_tol, cos_tol=None,
             normals=None, mask=None, weights=None, iters=0, min_count=6, damping=0.0):
    """the host program on a batch: depth [B,H,W] or points [B,3,H,W]; mp, mn [B,3,Hm,Wm], mv [B,Hm,Wm]; T [NT,3,4] -> dict of its outputs"""
    frame = np.ascontiguousarray(depth if points is None else points, F)
    B, (H, W) = frame.shape[0], frame.shape[-2:]
    Hm, Wm = mv.shape[-2:]
    n = H * W
    T = np.ascontiguousarray(T, F).reshape(-1, 3, 4)
    params = np.zeros((B, 16), F) if params is None else np.ascontiguousarray(params, F)
    mf = list(models_frame) if models_frame is not None else [PINHOLE] * B
    args = ["run", B, H, W, Hm, Wm, T.shape[0], int(points is not None), int(mask is not None), int(weights is not None), int(normals is not None),
            int(cos_tol is not None), f32_bits(dist_tol), f32_bits(cos_tol if cos_tol is not None else 0.0), iters, min_count, f64_bits(damping)]
    args += mf + list(models_model)
    blobs = [frame.tobytes(), params.tobytes()]
    blobs += [np.ascontiguousarray(mask, np.uint8).tobytes()] if mask is not None else []
    blobs += [np.ascontiguousarray(weights, F).tobytes()] if weights is not None else []
    blobs += [np.ascontiguousarray(normals, F).tobytes()] if normals is not None else []
    blobs += [np.ascontiguousarray(mp, F).tobytes(), np.ascontiguousarray(mn, F).tobytes(), np.ascontiguousarray(mv, np.uint8).tobytes(),
              np.ascontiguousarray(params_model, F).tobytes(), T.tobytes()]
    K = max(iters, 1)
    sizes = [B * n, 4 * B * n, 24 * B * n, 12 * B * n, 8 * B * n, 8 * K * B * 32] + ([8 * K * B * 6, K * B, 4 * K * B * 12] if iters else [])
    out = host_program.run(exe, args, blobs, sizes)
    r = dict(matched=np.frombuffer(out[0], np.uint8).reshape(B, H, W).astype(bool), residual=np.frombuffer(out[1], F).reshape(B, H, W),
             rows=np.frombuffer(out[2], F).reshape(B, 6, H, W), p=np.frombuffer(out[3], F).reshape(B, 3, H, W),
             uv=np.frombuffer(out[4], F).reshape(B, 2, H, W), systems=np.frombuffer(out[5], np.float64).reshape(K, B, 32))
    if iters:
        r.update(x=np.frombuffer(out[6], np.float64).reshape(K, B, 6), status=np.frombuffer(out[7], np.uint8).reshape(K, B),
                 Ts=np.frombuffer(out[8], F).reshape(K, B, 3, 4))
    return r


def host_scene(exe, s, T=None, iters=0, **kw):
    return host_run(exe, depth=s["depth"][None], params=s["row"][None], models_frame=[PINHOLE], mp=s["mp"][None], mn=s["mn"][None], mv=s["mv"][None],
                    params_model=s["row_model"][None], models_model=[PINHOLE], T=(s["T0"] if T is None else T)[None], dist_tol=s["dist_tol"],
                    iters=iters, **kw)


def host_solve(exe, S, T, damping=0.0, min_count=6):
    S, T = np.ascontiguousarray(S, np.float64).reshape(-1, 32), np.ascontiguousarray(T, F).reshape(-1, 3, 4)
    B = S.shape[0]
    out = host_program.run(exe, ["solve", B, min_count, f64_bits(damping)], [S.tobytes(), T.tobytes()], [48 * B, 48 * B, B])
    return np.frombuffer(out[0], F).reshape(B, 3, 4), np.frombuffer(out[1], np.float64).reshape(B, 6), np.frombuffer(out[2], np.uint8)


# ---- a batch of mixed cameras for the fused-against-composition tests ------------------------------------------------------------------

def mixed_case(frame_models, model_models, H=29, W=41, Hm=37, Wm=53, seed=0, per_image=True):
    """B images of the corner: a noisy pinhole depth of view B with a hole, lifted through frame_models[b] whatever that model is, against
    the pinhole maps of view A projected through model_models[b], from a T near the truth -- geometry that agrees only roughly, which is
    what a matrix of bit comparisons needs: every gate decides both ways.  Random invalid model pixels, a patch of zero normals, and a
    mask, weights (some 0) and frame normals to switch on.  -> dict of numpy arrays"""
    g = np.random.RandomState(9700 + seed)
    B = len(frame_models)
    f, fm = 0.6 * W, 0.6 * Wm
    depth = np.stack([corner_view(POSE_B, H, W, f)[0] for _ in range(B)]).astype(F)
    depth *= (1 + 0.02 * g.standard_normal(depth.shape)).astype(F)
    depth[:, 2:5, 3:9] = 0                                            # a hole
    mp, mn = (np.stack([x] * B).astype(F) for x in corner_view(POSE_A, Hm, Wm, fm)[1:])
    mv = (g.uniform(size=(B, Hm, Wm)) > 0.1).astype(np.uint8)
    mn[:, :, 5:8, 10:14] = 0                                          # zero normals inside valid pixels
    T = np.stack([(pose(0.02 * g.standard_normal(3), 0.03 * g.standard_normal(3)) @ CORNER_TRUTH)[:3] for _ in range(B if per_image else 1)]).astype(F)
    normals = np.stack([corner_view(POSE_B, H, W, f)[2]] * B).astype(F)
    return dict(B=B, H=H, W=W, Hm=Hm, Wm=Wm, depth=depth, params=np.stack([tc.row_for(m, H, W, f) for m in frame_models]),
                models_frame=list(frame_models), mp=mp, mn=mn, mv=mv, params_model=np.stack([tc.row_for(m, Hm, Wm, fm) for m in model_models]),
                models_model=list(model_models), T=T, dist_tol=0.25, mask=(g.uniform(size=(B, H, W)) > 0.1).astype(np.uint8),
                weights=np.where(g.uniform(size=(B, H, W)) > 0.05, g.uniform(0.5, 2.0, size=(B, H, W)), 0).astype(F), normals=normals, cos_tol=0.7)


def special_case():
    """NaN, +-inf, 0, -0.0 and negative values in the depth, the weights and T, zero and NaN normals and NaN points in the model maps, an
    image whose model maps are all invalid, and a T that puts every point behind the model camera: B = 5 pinhole images of 6 x 9"""
    c = mixed_case((PINHOLE,) * 5, (PINHOLE,) * 5, H=6, W=9, Hm=6, Wm=9, seed=3)
    d = c["depth"]
    d[0].reshape(-1)[:8] = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e38, 1e-38]
    c["weights"][0].reshape(-1)[8:14] = [np.nan, np.inf, -1.0, 0.0, -0.0, 1e-30]
    c["mn"][1, :, 2, :] = np.nan
    c["mp"][1, :, 3, :] = np.inf
    c["mv"][2] = 0
    c["T"][3] = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -10]], F)     # behind the model camera
    c["T"][4, 0, 0], c["T"][4, 1, 3] = np.nan, np.inf
    return c


def prepared(params, models):
    """a PreparedCamera on the GPU from numpy rows and model tags"""
    import torch
    from unidepth_amd import gtpoints
    return gtpoints.PreparedCamera(torch.from_numpy(np.array(params, np.float32, order="C")).cuda(), models)
