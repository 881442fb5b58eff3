"""Golden vectors of gt_points (unidepth_amd/gtpoints.py, csrc/reconstruct.hip): the reference's own Camera.reconstruct
(unidepth/utils/camera.py, torch on the CPU) on seeded inputs -> tests/golden/gt_points.npz.

    python tools/make_golden_gt_points.py          (needs the reference tree; only inputs, its outputs and measured errors are written)

This module also holds what the tests share: CASES / case_inputs(name) (seeded CPU torch.Generator inputs, uniform draws only, the
same bits on every machine) and an independent numpy restatement of ud_reconstruct (include/unidepth_hip.h UdReconstruct):
restate(..., dtype=np.float32) rounds every operation separately in fp32 -- the kernel's definition -- and
restate(..., dtype=np.float64) is the same expression in fp64, the value errors are measured from.
Nothing from the reference is imported at module import time.

The early exit of the OPENCV / Fisheye624 radial loop compares an image-wide maximum with 1e-3.  So that a library whose last bit
differs cannot flip that decision, case_inputs() settles every such camera: it scales the radial coefficients in small steps until
the fp32 restatement's largest |residual| lies outside [0.5e-3, 2e-3] at every iteration (settle()).  With that no test needs to
exclude a pixel.  main() additionally asserts that the reference takes the same number of iterations for every camera.

Tolerances are measured: for every stored case main() records the reference's own fp32 error against the fp64 restatement,
|d| / max(|truth|, 1e-4 max(|depth|, 1)) per point (error_ratio()), keeps the maximum per model in the npz ("referr.<model>") and
prints it; the kernel's bar per model is max(4 x that, 8 x 2^-24) (bar())."""
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gt_points.npz")

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = 1, 2, 3, 4, 5, 6
MODEL_NAMES = {PINHOLE: "Pinhole", EUCM: "EUCM", SPHERICAL: "Spherical", OPENCV: "OPENCV", FISHEYE624: "Fisheye624", MEI: "MEI"}
N_PARAMS = {PINHOLE: 4, EUCM: 6, SPHERICAL: 8, OPENCV: 16, FISHEYE624: 16, MEI: 9}
ITERATIVE = (OPENCV, FISHEYE624)
MARGIN = (0.5e-3, 2e-3)

# name -> (H, W, [(model, parameter list)] one per camera, B).  len(cameras) == B, or 1 camera broadcast over B images.
# f = focal lengths chosen for the field of view the path needs at the case's size; c = a principal point off the centre.
CASES = {
    "pinhole_5x7_b2": (5, 7, [(PINHOLE, [6.3, 6.1, 3.4, 2.6]), (PINHOLE, [11.0, 12.5, 2.9, 2.2])], 2),
    "eucm_9x29_b2": (9, 29, [(EUCM, [14.0, 14.5, 14.2, 4.3, 0.35, 1.2]),                    # alpha below 0.5
                             (EUCM, [9.0, 9.5, 15.1, 4.8, 0.72, 0.9])], 2),                 # alpha above 0.5
    "spherical_37x53_b2": (37, 53, [(SPHERICAL, [8.4, 11.8, 26.5, 18.5, 53.0, 37.0, math.pi, math.pi / 2]),   # the full panorama
                                    (SPHERICAL, [8.4, 11.8, 9.5, 4.5, 41.0, 29.0, 1.1, 0.62])], 2),   # a crop: smaller W, H and fields of view
    # one weakly distorted camera that leaves the radial loop after one or two iterations beside a strongly distorted one that runs longer
    "opencv_37x53_b2_iters": (37, 53, [(OPENCV, [62.0, 61.0, 26.1, 18.9, -0.02, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]),
                                       (OPENCV, [38.0, 39.0, 27.3, 17.8, -0.28, 0.09, -0.01, 0, 0, 0, 0, 0, 0, 0, 0, 0])], 2),
    # tangential and thin prism without radial terms (the Jacobian of that Newton loop starts from a matrix of ones in the reference), then
    # every term.  Thin prism WITHOUT tangential terms is not a case: the ones stay in the off-diagonals, the matrix is singular at the
    # principal point and whether a pixel ends as NaN depends on the last bit, in the reference as much as here.
    "opencv_9x29_b2_terms": (9, 29, [(OPENCV, [30.0, 31.0, 14.8, 4.2, 0, 0, 0, 0, 0, 0, -1.5e-3, 1e-3, 1e-3, 5e-4, -1e-3, 2e-4]),
                                     (OPENCV, [26.0, 27.0, 14.1, 4.9, -0.22, 0.07, -0.008, 0, 0, 0, 1e-3, -2e-3, 1e-3, 5e-4, -1e-3, 2e-4])], 2),
    "opencv_5x7_b2_tan": (5, 7, [(OPENCV, [8.0, 8.2, 3.3, 2.7, 0, 0, 0, 0, 0, 0, 2e-3, -1e-3, 5e-4, 1e-4, -5e-4, 1e-4]),   # tangential + prism, no radial
                                 (OPENCV, [7.0, 7.4, 3.6, 2.4, -0.2, 0.05, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])], 2),
    "fisheye624_9x29_b2": (9, 29, [(FISHEYE624, [18.0, 18.5, 14.6, 4.4, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 0, 0, 0, 0, 0, 0]),
                                   (FISHEYE624, [22.0, 21.0, 14.2, 4.7, -0.02, 0.01, -0.003, 0.001, 2e-4, 1e-5, 1e-3, -1e-3, 5e-4, 1e-4, -5e-4, 1e-4])], 2),
    "mei_37x53_b2": (37, 53, [(MEI, [60.0, 61.0, 26.2, 18.7, -0.1, 0.02, 0, 0, 1.0]),          # xi = 1 exactly
                              (MEI, [12.0, 12.5, 26.8, 18.1, -0.01, 0.001, 1e-3, -1e-3, 0.9])], 2),   # wide: pz < 1e-4 towards the corners
    "mixed_5x7_b6": (5, 7, [(PINHOLE, [6.0, 6.4, 3.5, 2.5]), (EUCM, [5.0, 5.2, 3.4, 2.6, 0.6, 1.1]),
                            (SPHERICAL, [1.1, 1.6, 3.5, 2.5, 7.0, 5.0, 2.8, 1.3]),
                            (OPENCV, [7.5, 7.7, 3.6, 2.4, -0.25, 0.08, -0.01, 0, 0, 0, 1e-3, -2e-3, 0, 0, 0, 0]),
                            (FISHEYE624, [5.0, 5.1, 3.3, 2.6, 0.04, -0.01, 0.002, -0.0004, 1e-4, -1e-5, 1e-3, -1e-3, 0, 0, 0, 0]),
                            (MEI, [6.0, 6.1, 3.5, 2.4, -0.1, 0.02, 1e-3, -1e-3, 0.8])], 6),
    "mixed_37x53_b6": (37, 53, [(OPENCV, [45.0, 46.0, 26.4, 18.3, -0.25, 0.08, -0.01, 0, 0, 0, 1e-3, -2e-3, 1e-3, 5e-4, -1e-3, 2e-4]),
                                (PINHOLE, [50.0, 51.0, 26.0, 18.0]), (MEI, [40.0, 41.0, 26.3, 18.6, -0.1, 0.02, 1e-3, -1e-3, 0.9]),
                                (FISHEYE624, [30.0, 30.5, 26.7, 18.2, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 0, 0, 0, 0, 0, 0]),
                                (SPHERICAL, [8.4, 11.8, 26.5, 18.5, 53.0, 37.0, 3.0, 1.4]), (EUCM, [30.0, 31.0, 26.2, 18.8, 0.45, 1.05])], 6),
    "broadcast_opencv_9x29_b3": (9, 29, [(OPENCV, [24.0, 25.0, 14.4, 4.6, -0.2, 0.06, -0.005, 0, 0, 0, 5e-4, -1e-3, 0, 0, 0, 0])], 3),
}


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _tanprism(ud, vd, p0, p1, s0, s1, s2, s3, use_tan, use_prism, iters, dt):
    """ud_cam_undistort_tanprism (csrc/camera_models.h), operation by operation."""
    xr, yr = ud.copy(), vd.copy()
    one, two, six = dt(1), dt(2), dt(6)
    for _ in range(iters):
        xr2, yr2 = xr * xr, yr * yr
        rd = xr2 + yr2
        ex, ey = xr, yr
        a = b = c = d = np.full_like(xr, one)
        if use_tan:
            ex = ex + ((two * xr2 + rd) * p0 + two * xr * yr * p1)
            ey = ey + ((two * yr2 + rd) * p1 + two * xr * yr * p0)
            a = one + six * xr * p0 + two * yr * p1
            b = two * (xr * p1 + yr * p0)
            c = b
            d = one + six * yr * p1 + two * xr * p0
        if use_prism:
            rd4 = rd * rd
            ex = ex + (s0 * rd + s1 * rd4)
            ey = ey + (s2 * rd + s3 * rd4)
            t1 = two * (s0 + two * s1 * rd)
            t2 = two * (s2 + two * s3 * rd)
            a = a + xr * t1
            b = b + yr * t1
            c = c + xr * t2
            d = d + yr * t2
        det = one / (a * d - b * c)
        e, f = ud - ex, vd - ey
        xr = xr + ((det * d) * e + (det * -b) * f)
        yr = yr + ((det * -c) * e + (det * a) * f)
    return xr, yr


def _radial(k, nk, th, dt):
    """ud_cam_radial: th (1 + sum k_j th^(2j+2)) and its derivative."""
    t2 = th * th
    pw, s, ds = t2, np.zeros_like(th), np.zeros_like(th)
    for j in range(nk):
        s = s + pw * k[j]
        ds = ds + (dt(2) * dt(j) + dt(3)) * k[j] * pw
        pw = pw * t2
    return (dt(1) + s) * th, dt(1) + ds


def _radial_step(k, nk, rnorm, th, delta, dt):
    """ud_cam_radial_step: one trust-region Newton iteration on theta."""
    eps = dt(np.float32(1e-3))
    thr, dth = _radial(k, nk, th, dt)
    res = thr - rnorm
    safe = np.where(np.abs(dth) < eps, eps, dth)
    step = -res / safe
    pred = -(res * step)
    sn = np.abs(step)
    step_scaled = np.where(sn > delta, step * (delta / sn), step)
    th_new = th + step_scaled
    res_new = _radial(k, nk, th_new, dt)[0] - rnorm
    actual = np.abs(res) - np.abs(res_new)
    rho = actual / pred
    rho = np.where((actual == 0) & (pred == 0), dt(1), rho)
    delta = np.where(rho > dt(0.5), np.minimum(dt(2) * delta, dt(1)), delta)
    delta = np.where(rho < dt(0.2), dt(0.25) * delta, delta)
    th = np.where(rho > dt(0.1), th_new, th)
    return th, delta


def _abs_sum(vals, dt):
    s = dt(0)
    for v in vals:
        s = dt(s + abs(v))
    return s


def _floor(x, m):
    """max(x, m) that lets a NaN through, as torch.clamp(min=m)."""
    return np.where(x < m, m, x)


def _solve_radial(p, model, uf, vf, dt):
    """(dx, dy, maxima, steps) of one OPENCV / Fisheye624 camera: the init / step / final launches of csrc/reconstruct.hip.  maxima[i] is
    the image-wide largest |residual| at theta_i that the loop looked at, steps the number of trust-region iterations it ran."""
    eps = dt(np.float32(1e-3))
    nk = 6 if model == FISHEYE624 else 3
    use_tan = _abs_sum(p[10:12], dt) > dt(np.float32(1e-6))
    use_prism = _abs_sum(p[12:16], dt) > dt(np.float32(1e-6))
    use_radial = _abs_sum(p[4:10], dt) > dt(np.float32(1e-6))
    ud, vd = (uf - p[2]) / p[0], (vf - p[3]) / p[1]
    xr, yr = _tanprism(ud, vd, p[10], p[11], p[12], p[13], p[14], p[15], use_tan, use_prism, 10 if (use_tan or use_prism) else 0, dt)
    rnorm = np.sqrt(xr * xr + yr * yr)
    th, delta = rnorm.copy(), np.full_like(rnorm, dt(0.1))
    maxima, steps = [], 0
    for _ in range(10 if use_radial else 0):
        r = np.abs(_radial(p[4:10], nk, th, dt)[0] - rnorm)
        m = float(np.max(r)) if not np.isnan(r).any() else float("nan")
        maxima.append(m)
        if m < eps:
            break
        steps += 1
        th, delta = _radial_step(p[4:10], nk, rnorm, th, delta, dt)
    close = (np.abs(th) < eps) & (np.abs(rnorm) < eps)
    sc = (np.tan(th) if model == FISHEYE624 else th) / rnorm
    return np.where(close, xr, sc * xr), np.where(close, yr, sc * yr), maxima, steps


def _mei(p, uf, vf, dt):
    """ud_cam_mei_dir: (dx, dy, pz), not normalised."""
    eps = dt(np.float32(1e-6))
    k1, k2, p0, p1, xi = p[4], p[5], p[6], p[7], p[8]
    use_radial = _abs_sum(p[4:6], dt) > eps
    use_tan = _abs_sum(p[6:8], dt) > eps
    ud, vd = (uf - p[2]) / p[0], (vf - p[3]) / p[1]
    z = dt(0)
    xr, yr = _tanprism(ud, vd, p0, p1, z, z, z, z, True, False, 20 if use_tan else 0, dt)
    rnorm = np.sqrt(xr * xr + yr * yr)
    th = rnorm.copy()
    for _ in range(20 if use_radial else 0):
        t2 = th * th
        t4 = t2 * t2
        thr = (dt(1) + k1 * t2 + k2 * t4) * th
        dth = dt(1) + dt(3) * k1 * t2 + dt(5) * k2 * t4
        step = (rnorm - thr) / dth
        step = np.where(np.abs(dth) > eps, step, np.sign(step) * eps * dt(10))
        th = th + step
    close = (np.abs(th) < eps) & (np.abs(rnorm) < eps)
    dx = np.where(close, xr, th * xr / rnorm)
    dy = np.where(close, yr, th * yr / rnorm)
    rho = np.sqrt(dx * dx + dy * dy)
    rho2 = rho * rho
    sq = np.sqrt(dt(1) + (dt(1) - xi * xi) * rho2)
    pz = dt(1) - xi * (rho2 + dt(1)) / (xi + sq)
    if xi == dt(1):
        pz = (dt(1) - rho2) / dt(2)
    return dx, dy, pz


def _base(x, y, z, d, dt):
    """Camera.reconstruct of the base class: rays / rays.z.clamp(1e-4) * depth.clamp(1e-4)."""
    zc, dc = _floor(z, dt(np.float32(1e-4))), _floor(d, dt(np.float32(1e-4)))
    return np.stack([x / zc * dc, y / zc * dc, z / zc * dc])


def restate(depth, params, models, dtype=np.float32, info=None):
    """ud_reconstruct: depth [B,1,H,W] or [B,H,W], params [B,16] (fp32 values), models [B] -> points [B,3,H,W] in `dtype`, every
    operation rounded separately in `dtype`.  info (a dict) receives {"maxima": {b: [...]}, "steps": {b: n}} of the iterative images."""
    dt = np.dtype(dtype).type
    depth = np.asarray(depth, dtype=np.float32)
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    depth = depth.reshape(B, H, W).astype(dtype)
    params = np.asarray(params, dtype=np.float32).reshape(B, 16).astype(dtype)
    uf = np.broadcast_to(np.arange(W).astype(dtype) + dt(0.5), (H, W)).copy()
    vf = np.broadcast_to((np.arange(H).astype(dtype) + dt(0.5))[:, None], (H, W)).copy()
    out = np.zeros((B, 3, H, W), dtype=dtype)
    c1e5, c1e3 = dt(np.float32(1e-5)), dt(np.float32(1e-3))
    with np.errstate(all="ignore"):
        for b in range(B):
            p, d, m = params[b], depth[b], int(models[b])
            if m == PINHOLE:
                x = (uf - p[2]) / p[0]
                y = (vf - p[3]) / p[1]
                z = np.full_like(x, dt(0) * (p[0] + p[1] + p[2] + p[3]) + dt(1))      # 1, or NaN with a NaN intrinsic
                zc, dc = _floor(z, dt(np.float32(1e-4))), _floor(d, dt(0))
                out[b] = np.stack([x / zc * dc, y / zc * dc, z / zc * dc])
            elif m == EUCM:
                al, be = p[4], p[5]
                mx, my = (uf - p[2]) / p[0], (vf - p[3]) / p[1]
                r2 = mx * mx + my * my
                sv = dt(1) - (dt(2) * al - dt(1)) * be * r2
                mz = (dt(1) - be * (al * al) * r2) / (al * np.sqrt(_floor(sv, c1e5)) + (dt(1) - al))
                cf = dt(1) / np.sqrt(mx * mx + my * my + mz * mz + c1e5)
                out[b] = _base(cf * mx, cf * my, _floor(cf * mz, c1e3), d, dt)
            elif m == SPHERICAL:
                lon = (uf - (p[4] - dt(1)) / dt(2)) / (p[4] - dt(1)) * (dt(2) * p[6])
                lat = (vf - (p[5] - dt(1)) / dt(2)) / (p[5] - dt(1)) * (dt(2) * p[7])
                cl = np.cos(lat)
                x, y, z = cl * np.sin(lon), np.sin(lat), cl * np.cos(lon)
                n = _floor(np.sqrt(x * x + y * y + z * z), c1e5)
                out[b] = np.stack([x / n * d, y / n * d, z / n * d])
            elif m in ITERATIVE:
                dx, dy, maxima, steps = _solve_radial(p, m, uf, vf, dt)
                if info is not None:
                    info.setdefault("maxima", {})[b] = maxima
                    info.setdefault("steps", {})[b] = steps
                out[b] = _base(dx, dy, np.ones_like(dx), d, dt)
            elif m == MEI:
                dx, dy, pz = _mei(p, uf, vf, dt)
                out[b] = _base(dx, dy, pz, d, dt)
            else:
                raise ValueError(f"model tag {m}")
    return out


def error_ratio(delta, truth, depth):
    """|delta| / max(|truth|, 1e-4 max(|depth|, 1)) per point component, fp64; NaN positions of the truth give 0 (they are compared
    separately: they must match exactly)."""
    B = truth.shape[0]
    d = np.abs(np.asarray(depth, dtype=np.float64).reshape(B, 1, truth.shape[-2], truth.shape[-1]))
    den = np.maximum(np.abs(truth.astype(np.float64)), 1e-4 * np.maximum(np.nan_to_num(d, nan=1.0), 1.0))
    with np.errstate(invalid="ignore"):
        r = np.abs(delta.astype(np.float64)) / den
    return np.where(np.isnan(truth), 0.0, r)


def bar(ref_err: float) -> float:
    """The kernel's bar for a model whose reference error was measured as ref_err."""
    return max(4.0 * float(ref_err), 8.0 * 2.0 ** -24)


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def margins_ok(maxima):
    return all(not (MARGIN[0] <= m <= MARGIN[1]) for m in maxima)


@functools.lru_cache(maxsize=None)
def settle(model, params, H, W):
    """The parameters of an OPENCV / Fisheye624 camera with the radial coefficients scaled by (1 + 0.03 j), the smallest j at which the
    fp32 restatement's image-wide residual maximum avoids MARGIN at every iteration."""
    base = np.zeros(16, dtype=np.float32)
    base[: len(params)] = params
    for j in range(64):
        p = base.copy()
        p[4:10] = (base[4:10] * np.float32(1.0 + 0.03 * j)).astype(np.float32)
        info = {}
        restate(np.ones((1, H, W), np.float32), p[None], [model], np.float32, info)
        if margins_ok(info.get("maxima", {}).get(0, [])):
            return tuple(float(v) for v in p)
    raise AssertionError(f"no scaling of {params} keeps the residual maxima out of {MARGIN}")


def case_inputs(name):
    """(depth fp32 [B,1,H,W], params fp32 [n,16] zero-padded, models [n]) of a case, numpy; n = B, or 1 for a broadcast camera."""
    H, W, cams, B = CASES[name]
    g = torch.Generator().manual_seed(5200 + sorted(CASES).index(name))
    depth = (0.2 + 19.8 * torch.rand(B, 1, H, W, generator=g)).float().numpy()
    depth[0, 0, 0, 0] = 0.0
    depth[0, 0, 0, 1] = -1.5
    depth[0, 0, 0, 2] = 5e-5                                  # below the 1e-4 floor
    depth[0, 0, 1, 0] = np.nan
    depth[B - 1, 0, H - 1, W - 1] = -0.25
    depth[B - 1, 0, H - 1, W - 2] = 0.0
    depth[B - 1, 0, H - 2, W - 1] = 2e-5
    params = np.zeros((len(cams), 16), dtype=np.float32)
    for i, (m, p) in enumerate(cams):
        assert len(p) == N_PARAMS[m]
        params[i, : len(p)] = settle(m, tuple(p), H, W) if m in ITERATIVE else p
    return depth, params, [m for m, _ in cams]


def case_rows(name):
    """case_inputs with the camera rows expanded to the batch: (depth, params [B,16], models [B])."""
    depth, params, models = case_inputs(name)
    B = depth.shape[0]
    if params.shape[0] != B:
        params, models = np.repeat(params, B, axis=0), models * B
    return depth, params, models


def make_camera(ns, model, row):
    """A camera object of namespace `ns` (unidepth_amd.cameras or the reference's utils.camera) from one zero-padded row."""
    p = torch.tensor(np.asarray(row[: N_PARAMS[model]], dtype=np.float32))
    cls = getattr(ns, MODEL_NAMES[model])
    return cls(params=p[None]) if model == PINHOLE else cls(p[None] if ns.__name__.startswith("unidepth_amd") else p)


def case_camera(ns, name):
    """The camera of a case from unidepth_amd.cameras' classes (`ns`): the single camera of a broadcast case, else a BatchCamera."""
    _, params, models = case_inputs(name)
    cams = [make_camera(ns, m, r) for m, r in zip(models, params)]
    return cams[0] if len(cams) == 1 else ns.BatchCamera(cams)


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_module():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import warnings
    from oracle import ref_loader
    warnings.simplefilter("ignore")
    ref_loader._prepare()
    import unidepth.utils.camera as rc
    return rc


def reference_output(rc, name):
    """(points fp32 [B,3,H,W], iterations of the radial loop per image or -1) of a case from the reference's own reconstruct: a single
    camera is called with the whole batch (it broadcasts), several cameras go through the reference's BatchCamera."""
    depth, params, models = case_inputs(name)
    B = depth.shape[0]
    cams = [make_camera(rc, m, r) for m, r in zip(models, params)]
    d = torch.from_numpy(depth)
    steps, seen = [], []
    real_max = torch.max

    def counting_max(*a, **k):                                # the loop's `torch.max(torch.abs(residual))`: one call per look
        v = real_max(*a, **k)
        if isinstance(v, torch.Tensor) and v.ndim == 0:
            seen.append(float(v))
        return v

    outs = []
    torch.max = counting_max
    try:
        if len(cams) == 1:
            outs.append(cams[0].reconstruct(d))
            looks = [list(seen)] * B
        else:
            batch = rc.Camera._stack_or_cat_cameras(cams, torch.cat, dim=0)
            assert type(batch).__name__ == "BatchCamera" and len(batch) == B
            looks = []
            for i, cam in enumerate(batch.cameras):           # BatchCamera.reconstruct, member by member, to count each member's looks
                del seen[:]
                outs.append(cam.reconstruct(d[i:i + 1]))
                looks.append(list(seen))
            whole = batch.reconstruct(d)
    finally:
        torch.max = real_max
    out = torch.cat(outs)
    if len(cams) > 1:
        assert torch.equal(torch.nan_to_num(whole, nan=-7.0), torch.nan_to_num(out, nan=-7.0))
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3, depth.shape[-2], depth.shape[-1])
    for b in range(B):
        m = models[b if len(cams) > 1 else 0]
        lk = looks[b]
        steps.append((len(lk) - 1 if lk and lk[-1] < 1e-3 else len(lk)) if m in ITERATIVE else -1)
    return out.numpy(), steps


def main():
    rc = reference_module()
    out, referr = {}, {}
    for name in CASES:
        depth, params, models = case_rows(name)
        ref, ref_steps = reference_output(rc, name)
        info = {}
        r32 = restate(depth, params, models, np.float32, info)
        truth = restate(depth, params, models, np.float64)
        assert np.array_equal(np.isnan(ref), np.isnan(truth)) and np.array_equal(np.isnan(r32), np.isnan(truth)), name
        for b, m in enumerate(models):
            if m in ITERATIVE:
                assert margins_ok(info.get("maxima", {}).get(b, [])), (name, b, info["maxima"][b])
                assert info.get("steps", {}).get(b, 0) == ref_steps[b], (name, b, info.get("steps"), ref_steps)
        e_ref = error_ratio(ref - truth, truth, depth)
        e_r32 = error_ratio(r32 - truth, truth, depth)
        for b, m in enumerate(models):
            referr[m] = max(referr.get(m, 0.0), float(e_ref[b].max()))
        steps32 = [info.get("steps", {}).get(b, -1) for b in range(len(models))]
        print(f"{name:28s} reference error {e_ref.max():.3e}  fp32 restatement error {e_r32.max():.3e}  "
              f"restatement vs reference {error_ratio(r32 - ref, truth, depth).max():.3e}  iterations {steps32}")
        out[name + ".depth"], out[name + ".params"], out[name + ".models"] = depth, params, np.asarray(models, dtype=np.int32)
        out[name + ".out"], out[name + ".steps"] = ref, np.asarray(ref_steps, dtype=np.int32)
    for m, e in sorted(referr.items()):
        out["referr." + MODEL_NAMES[m]] = np.float64(e)
        print(f"referr.{MODEL_NAMES[m]:11s} {e:.3e}   bar {bar(e):.3e}")
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
