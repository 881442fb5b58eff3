"""Golden vectors of project_camera / render_depth_camera (unidepth_amd/reproject.py, csrc/project.hip, csrc/splat.hip): the reference's
own Camera.project (unidepth/utils/camera.py, torch on the CPU) on seeded points -> tests/golden/camera_project.npz.

    python tools/make_golden_camera_project.py     (needs the reference tree; only inputs, its outputs and measured errors are written)

This module also holds what the tests share: CASES / case_inputs(name) (the camera rows of tools/make_golden_gt_points.py's cases with
seeded points, uniform draws only, the same bits on every machine) and an independent numpy restatement of ud_camera_project and
ud_splat_camera (include/unidepth_hip.h): project(..., dtype=np.float32) rounds every operation separately in fp32 -- the kernels'
definition -- and project(..., dtype=np.float64) is the same expression in fp64, the value errors are measured from; render() is the
splat on top of it.  Nothing from the reference is imported at module import time.

The points of a case come in two groups.  REGULAR points spread over and somewhat beyond the camera's field of view with depths in
[0.5, 5]; they are redrawn until the fp64 restatement keeps every one of them well conditioned (well_conditioned(): z >= 0.05 except
for Spherical, whose points keep |sin(latitude)| <= 0.97 instead, every clamped denominator at least twice its clamp, u and v within a quarter of the image's size of the image and at least MARGIN away from every multiple of 0.5, which covers 0, W, H and the
cell borders with pixel_offset 0 or 0.5).  main() asserts MARGIN >= 8 x the largest bar expressed in pixels (the measured bars reach
1.2e-3 px at the largest |uv|, hence 1e-2 px), so masks and cells are decided by the definition and not by a last bit, and no test
excludes a point.  SPECIAL points (z = 0, z < 0, the axis, NaN and
infinite components, points behind the camera) sit at the end of every image and are compared against the fp32 restatement only.

Tolerances are measured: main() records for each model the largest |uv_ref - uv_fp64| / max(|uv_fp64|, 1) of the reference's own fp32
output over the regular points ("referr.<model>"); the kernel's bar is make_golden_gt_points.bar() = max(4 x that, 8 x 2^-24).  The
values are stored in the npz and printed into profiles/camera_project_bars.txt."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_project.npz")
BARS_TXT = os.path.join(ROOT, "profiles", "camera_project_bars.txt")

_spec = importlib.util.spec_from_file_location("make_golden_gt_points", os.path.join(ROOT, "tools", "make_golden_gt_points.py"))
gp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gp)

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = gp.PINHOLE, gp.EUCM, gp.SPHERICAL, gp.OPENCV, gp.FISHEYE624, gp.MEI
MODEL_NAMES, bar = gp.MODEL_NAMES, gp.bar
MARGIN = 1e-2                                                  # pixels; see main(): at least 8 x the largest bar in pixels
# the camera rows of these gt_points cases: every size, B = 2 of every model, both mixed batches, the broadcast camera
CASES = tuple(gp.CASES)
SPECIAL = np.array([[0.3, -0.2, 0.0], [0.0, 0.0, 0.0], [0.4, 0.1, -1.0], [-0.3, 0.2, -2.5], [0.0, 0.0, 1.5], [0.0, 0.0, -1.5],
                    [np.nan, 0.1, 1.0], [0.1, np.nan, 2.0], [0.1, 0.2, np.nan], [np.inf, 0.1, 1.0], [0.1, -np.inf, 1.0], [0.1, 0.2, np.inf],
                    [0.2, 0.1, 5e-10], [0.2, 0.1, -5e-10], [3.0, -2.0, 1e-3]], dtype=np.float32)


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _floor(x, m):
    """max(x, m) that lets a NaN through, as torch.clamp(min=m)."""
    return np.where(x < m, m, x)


def _back(p, xr, yr, p0, p1, s, dt):
    """ud_cam_project_back: tangential, thin prism (s = None for MEI), focal lengths and principal point."""
    two = dt(2)
    xr2, yr2 = xr * xr, yr * yr
    rd = xr2 + yr2
    ud = xr + ((two * xr2 + rd) * p0 + two * xr * yr * p1)
    vd = yr + ((two * yr2 + rd) * p1 + two * xr * yr * p0)
    if s is not None:
        rd4 = rd * rd
        ud = ud + (s[0] * rd + s[1] * rd4)
        vd = vd + (s[2] * rd + s[3] * rd4)
    return ud * p[0] + p[2], vd * p[1] + p[3]


def _front(x, y, z, dt):
    """ud_cam_project_front: z -> 1e-9 sign(z) when |z| < 1e-9, ab = xy / z, r = |ab|."""
    eps = dt(np.float32(1e-9))
    sg = np.where(z > 0, dt(1), np.where(z < 0, dt(-1), dt(0))).astype(z.dtype)
    zz = np.where(np.abs(z) < eps, eps * sg, z)
    a, b = x / zz, y / zz
    return a, b, np.sqrt(a * a + b * b)


def project_model(m, p, x, y, z, dt, cond=None):
    """(u, v) of one camera: ud_cam_project_<model> (csrc/camera_models.h), operation by operation.  cond (a list) receives the ratios
    clamped denominator / clamp of the models that clamp."""
    one, two = dt(1), dt(2)
    c = lambda v: dt(np.float32(v))
    if m == PINHOLE:
        zc = _floor(z, c(0.01))
        if cond is not None:
            cond.append(z / c(0.01))
        return (p[0] * x + p[2] * z) / zc, (p[1] * y + p[3] * z) / zc
    if m == EUCM:
        al, be = p[4], p[5]
        d = np.sqrt(be * (x * x + y * y) + z * z)
        raw = al * d + (one - al) * z
        den = _floor(raw, c(1e-3))
        if cond is not None:
            cond.append(raw / c(1e-3))
        return p[0] * (x / den) + p[2], p[1] * (y / den) + p[3]
    if m == SPHERICAL:
        lon = np.arctan2(x, z)
        n = np.sqrt(x * x + y * y + z * z)
        if cond is not None:
            cond.append(n / c(1e-5))
        lat = np.arcsin(y / _floor(n, c(1e-5)))
        return (lon / (two * p[6]) * (p[4] - one) + (p[4] - one) / two, lat / (two * p[7]) * (p[5] - one) + (p[5] - one) / two)
    if m == OPENCV:
        a, b, r = _front(x, y, z, dt)
        r2 = r * r
        r4 = r2 * r2
        r6 = r4 * r2
        num = one + ((r2 * p[4] + r4 * p[5]) + r6 * p[6])
        return _back(p, a * num, b * num, p[10], p[11], p[12:16], dt)
    if m == FISHEYE624:
        a, b, r = _front(x, y, z, dt)
        th = np.arctan(r)
        small = r < c(1e-9)
        dx, dy = np.where(small, one, a / r), np.where(small, one, b / r)
        t2 = th * th
        pw, s = th * t2, np.zeros_like(th)
        for j in range(6):
            s = s + pw * p[4 + j]
            pw = pw * t2
        thk = th + s
        return _back(p, thk * dx, thk * dy, p[10], p[11], p[12:16], dt)
    if m == MEI:
        n = np.sqrt(x * x + y * y + z * z)
        den = z + p[8] * n
        a, b = x / den, y / den
        r = np.sqrt(a * a + b * b)
        r2 = r * r
        r4 = r2 * r2
        f = one + p[4] * r2 + p[5] * r4
        return _back(p, a * f, b * f, p[6], p[7], None, dt)
    raise ValueError(f"model tag {m}")


def _transform(x, y, z, t):
    return [((t[r, 0] * x + t[r, 1] * y) + t[r, 2] * z) + t[r, 3] for r in range(3)]


def inside_model(m, u, v, z, H, W):
    """ud_cam_inside: each class's own test, comparisons taken literally (NaN behaves as in the reference)."""
    with np.errstate(invalid="ignore"):
        if m == PINHOLE:
            return (u >= 0) & (u < W) & (v >= 0) & (v < H)
        out = (u < 0) | (u > W) | (v < 0) | (v > H)
        if m == EUCM:
            out = out | (z < 0)
        return ~out


def project(xyz, params, models, image_shape, T=None, dtype=np.float32, cond=None):
    """ud_camera_project: xyz [B,N,3], params [B,16] (fp32 values), models [B], T None / [nT,3,4] -> (uv [B,N,2], inside bool [B,N],
    depth [B,N]) in `dtype`, every operation rounded separately.  cond (a dict) receives b -> the list of clamp ratios of image b."""
    dt = np.dtype(dtype).type
    H, W = image_shape
    xyz = np.asarray(xyz, dtype=np.float32).astype(dtype)
    B, N = xyz.shape[:2]
    params = np.asarray(params, dtype=np.float32).reshape(B, 16).astype(dtype)
    T = None if T is None else np.asarray(T, dtype=np.float32).reshape(-1, 3, 4).astype(dtype)
    uv, inside, depth = np.zeros((B, N, 2), dtype), np.zeros((B, N), bool), np.zeros((B, N), dtype)
    with np.errstate(all="ignore"):
        for b in range(B):
            x, y, z = (np.ascontiguousarray(xyz[b, :, k]) for k in range(3))
            if T is not None:
                x, y, z = _transform(x, y, z, T[b if T.shape[0] > 1 else 0])
            m = int(models[b])
            cl = [] if cond is not None else None
            u, v = project_model(m, params[b], x, y, z, dt, cl)
            if cond is not None:
                cond[b] = cl
            uv[b, :, 0], uv[b, :, 1] = u, v
            inside[b] = inside_model(m, u, v, z, H, W)
            depth[b] = np.sqrt(x * x + y * y + z * z) if m == SPHERICAL else z
    assert uv.dtype == dtype and depth.dtype == dtype
    return uv, inside, depth


def render(xyz, params, models, image_shape, T=None, mode="nearest", pixel_offset=0.0, rounding="floor", depth_range=None, cos_limit=None,
           colors=None, dtype=np.float32):
    """ud_splat_camera restated on per-image clouds (xyz: [B,N,3] or a list of [n_b,3]) -> dict of depth [B,H,W] (fp32 bits of the winner
    in nearest mode, the float64 mean in mean mode), index, count int32 [B,H,W], rgb [B,3,H,W] or None, kept: list of bool [n_b]."""
    dt = np.dtype(dtype).type
    H, W = image_shape
    B = len(xyz)
    params = np.asarray(params, dtype=np.float32).reshape(B, 16)
    depth = np.zeros((B, H * W), dtype=np.float32 if mode == "nearest" else np.float64)
    index = np.full((B, H * W), -1, dtype=np.int32)
    count = np.zeros((B, H * W), dtype=np.int32)
    rgb = None if colors is None else np.zeros((B, 3, H * W), dtype=np.asarray(colors[0]).dtype)
    kept = []
    Ts = None if T is None else np.asarray(T, dtype=np.float32).reshape(-1, 3, 4)
    for b in range(B):
        cloud = np.asarray(xyz[b], dtype=np.float32)[None]
        m = int(models[b])
        Tb = None if T is None else Ts[b:b + 1] if len(Ts) > 1 else Ts
        uv, _, dep = project(cloud, params[b:b + 1], [m], image_shape, Tb, dtype)
        with np.errstate(all="ignore"):
            x, y, z = (cloud[0, :, k].astype(dtype) for k in range(3))
            if Tb is not None:
                x, y, z = _transform(x, y, z, Tb[0].astype(dtype))
            n = np.sqrt(x * x + y * y + z * z)
            keep = np.ones(x.shape, bool)
            if m != SPHERICAL:
                keep &= ~(z <= 0)
            if m == MEI:
                keep &= (z + params[b, 8].astype(dtype) * n) > 0
            if cos_limit is not None:
                keep &= z >= dt(np.float32(cos_limit)) * n
            dep = dep[0]
            idx = []
            for c, size in ((uv[0, :, 0] + dt(np.float32(pixel_offset)), W), (uv[0, :, 1] + dt(np.float32(pixel_offset)), H)):
                f = np.trunc(c) if rounding == "trunc" else np.floor(c)
                good = (f >= 0) & (f < 2147483648.0)
                i = np.where(good, f, 0).astype(np.int64)
                keep &= good & (i < size)
                idx.append(i)
            if depth_range is not None:
                keep &= (dep >= dt(np.float32(depth_range[0]))) & (dep <= dt(np.float32(depth_range[1])))
            keep &= (dep > 0) if mode == "nearest" else (np.abs(dep) <= 2.0 ** 20)
        kept.append(keep)
        r = np.nonzero(keep)[0]
        pk, zk = (idx[1] * W + idx[0])[r], dep[r]
        count[b] = np.bincount(pk, minlength=H * W)
        if mode == "nearest":
            zk = zk.astype(np.float32)
            order = np.lexsort((r, zk.view(np.uint32), pk))
            first = order[np.concatenate([[True], pk[order][1:] != pk[order][:-1]])] if r.size else order
            depth[b, pk[first]] = zk[first]
            index[b, pk[first]] = r[first]
            if rgb is not None:
                rgb[b][:, pk[first]] = np.asarray(colors[b])[r[first]].T
        else:
            s = np.bincount(pk, weights=zk.astype(np.float64), minlength=H * W)
            depth[b] = np.where(count[b] > 0, s / np.maximum(count[b], 1), 0.0)
    shape = (B, H, W)
    return {"depth": depth.reshape(shape), "index": index.reshape(shape), "count": count.reshape(shape),
            "rgb": None if rgb is None else rgb.reshape(B, 3, H, W), "kept": kept}


def uv_error(delta, truth):
    """|delta| / max(|truth|, 1) per coordinate, fp64; NaN positions of the truth give 0 (they are compared separately)."""
    with np.errstate(invalid="ignore"):
        r = np.abs(delta.astype(np.float64)) / np.maximum(np.abs(truth.astype(np.float64)), 1.0)
    return np.where(np.isnan(truth), 0.0, r)


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def well_conditioned(xyz, params, model, image_shape):
    """bool [N]: the fp64 restatement keeps the point clear of every decision (see the module docstring)."""
    cond = {}
    uv, _, _ = project(xyz[None], params[None], [model], image_shape, None, np.float64, cond)
    ok = np.ones(len(xyz), bool) if model == SPHERICAL else xyz[:, 2].astype(np.float64) >= 0.05      # a panorama sees behind itself
    for ratio in cond[0]:
        ok &= ratio >= 2.0
    half = uv[0] * 2.0
    ok &= (np.abs(half - np.rint(half)) >= 2.0 * MARGIN).all(axis=1)
    ok &= np.isfinite(uv[0]).all(axis=1)
    if model == SPHERICAL:                                    # asin near the poles multiplies the rounding of its argument by 1 / cos(lat)
        d = xyz.astype(np.float64)
        ok &= np.abs(d[:, 1]) <= 0.97 * np.linalg.norm(d, axis=1)
    H, W = image_shape                                        # "somewhat beyond": at most a quarter of the image's size outside it
    ok &= (uv[0, :, 0] > -0.25 * W) & (uv[0, :, 0] < 1.25 * W) & (uv[0, :, 1] > -0.25 * H) & (uv[0, :, 1] < 1.25 * H)
    return ok


def _half_angle(model, row, H, W):
    """the largest angle off the axis of the image's border, from the fp64 restatement of gt_points at unit depth"""
    pts = gp.restate(np.ones((1, 1, H, W), np.float32), row[None], [model], np.float64)[0]
    border = np.concatenate([pts[:, 0, :], pts[:, -1, :], pts[:, :, 0], pts[:, :, -1]], axis=1)
    cosang = border[2] / np.linalg.norm(border, axis=0)
    return float(np.arccos(np.clip(np.nanmin(cosang), -1.0, 1.0)))


def _draw(g, model, row, H, W, n):
    """n candidate points of one camera, fp32: directions over 1.15 x the field of view (uniform draws only), depths in [0.5, 5]"""
    u1, u2, u3 = (torch.rand(n, generator=g).double().numpy() for _ in range(3))
    depth = 0.5 + 4.5 * u3
    if model == SPHERICAL:
        lon = (2 * u1 - 1) * min(1.15 * float(row[6]), math.pi * 0.999)
        lat = (2 * u2 - 1) * min(1.15 * float(row[7]), math.pi / 2 * 0.98)
        d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=1)
        return (d * depth[:, None]).astype(np.float32)
    th = u1 * min(1.15 * _half_angle(model, row, H, W), math.radians(80.0))
    ph = 2 * math.pi * u2
    d = np.stack([np.tan(th) * np.cos(ph), np.tan(th) * np.sin(ph), np.ones_like(th)], axis=1)
    return (d * depth[:, None]).astype(np.float32)


_CASE_CACHE = {}


def case_inputs(name):
    """(xyz fp32 [B,N,3] with N = H * W, params fp32 [B,16], models [B], n_regular): the regular points first, SPECIAL at the end of every
    image (as many of them as fit beside at least 20 regular points)."""
    if name in _CASE_CACHE:
        return _CASE_CACHE[name]
    H, W = gp.CASES[name][:2]
    _, params, models = gp.case_rows(name)
    B, N = len(models), H * W
    n_special = min(len(SPECIAL), N - 20)
    n_reg = N - n_special
    g = torch.Generator().manual_seed(7300 + sorted(gp.CASES).index(name))
    xyz = np.zeros((B, N, 3), dtype=np.float32)
    for b in range(B):
        got = np.zeros((0, 3), dtype=np.float32)
        for _ in range(64):
            cand = _draw(g, models[b], params[b], H, W, 2 * N)
            got = np.concatenate([got, cand[well_conditioned(cand, params[b], models[b], (H, W))]])
            if len(got) >= n_reg:
                break
        assert len(got) >= n_reg, (name, b, len(got))
        xyz[b, :n_reg] = got[:n_reg]
        xyz[b, n_reg:] = SPECIAL[:n_special]
    _CASE_CACHE[name] = (xyz, params, list(models), n_reg)
    return _CASE_CACHE[name]


def planar(xyz, H, W):
    """[B,N,3] rows -> the planar point map [B,3,H,W] of the same points (point r = pixel r)"""
    return np.ascontiguousarray(xyz.transpose(0, 2, 1)).reshape(xyz.shape[0], 3, H, W)


def roundtrip_cases():
    """the gt_points cases whose every pixel is valid for a round trip gt_points -> render_depth_camera: in the fp64 restatement every
    point of a positive-depth map is finite, in front of the camera where the model needs it, and projects back to within a quarter of
    a pixel of its own pixel's centre (the solvers of gt_points leave up to 1.4e-2 px in fp32).  Returns {name: depth fp32 [B,1,H,W]} (the case's seeded depths with the special values replaced by 1.25)."""
    out = {}
    for name in gp.CASES:
        depth, params, models = gp.case_rows(name)
        H, W = depth.shape[-2:]
        with np.errstate(invalid="ignore"):
            depth = np.where(np.isnan(depth) | (depth < 0.2), np.float32(1.25), depth).astype(np.float32)
        pts = gp.restate(depth, params, models, np.float64)
        rows = pts.reshape(len(models), 3, H * W).transpose(0, 2, 1)
        if not np.isfinite(rows).all():
            continue
        uv, _, dep = project(rows.astype(np.float32), params, models, (H, W), None, np.float64)
        cu, cv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        centre = np.stack([cu.ravel(), cv.ravel()], axis=1)[None]
        ok = (np.abs(uv - centre) <= 0.25).all() and (dep > 0).all()
        for b, m in enumerate(models):
            if m != SPHERICAL:
                ok = ok and (rows[b, :, 2] > 0.05).all()
        if ok:
            out[name] = depth
    return out


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_output(rc, name):
    """(uv fp32 [B,2,H,W], mask uint8 [B,1,H,W]: 0 / 1, or 2 where the class sets none) of a case from the reference's own project,
    member by member as its BatchCamera does"""
    xyz, params, models, _ = case_inputs(name)
    H, W = gp.CASES[name][:2]
    pts = torch.from_numpy(planar(xyz, H, W))
    uvs, masks = [], []
    for b, m in enumerate(models):
        cam = gp.make_camera(rc, m, params[b])
        uv = cam.project(pts[b:b + 1])
        mask = cam.get_projection_mask()
        assert uv.dtype == torch.float32 and tuple(uv.shape) == (1, 2, H, W)
        uvs.append(uv.numpy().copy())
        masks.append(np.full((1, 1, H, W), 2, np.uint8) if mask is None else mask.numpy().astype(np.uint8).reshape(1, 1, H, W))
    return np.concatenate(uvs), np.concatenate(masks)


def class_mask(model, inside):
    """what the class's get_projection_mask() returns for an `inside` array: Pinhole's is inverted, Spherical has none (2)"""
    if model == PINHOLE:
        return (~inside).astype(np.uint8)
    if model == SPHERICAL:
        return np.full(inside.shape, 2, np.uint8)
    return inside.astype(np.uint8)


def main():
    rc = gp.reference_module()
    out, referr, worst_px = {}, {}, {}
    lines = []
    for name in CASES:
        xyz, params, models, n_reg = case_inputs(name)
        H, W = gp.CASES[name][:2]
        ref_uv, ref_mask = reference_output(rc, name)
        uv32, in32, _ = project(xyz, params, models, (H, W), None, np.float32)
        uv64, in64, _ = project(xyz, params, models, (H, W), None, np.float64)
        ref_rows = ref_uv.reshape(len(models), 2, H * W).transpose(0, 2, 1)
        reg = slice(0, n_reg)
        assert np.isfinite(ref_rows[:, reg]).all() and np.isfinite(uv32[:, reg]).all(), name
        e_ref = uv_error(ref_rows[:, reg] - uv64[:, reg], uv64[:, reg])
        e_r32 = uv_error(uv32[:, reg] - uv64[:, reg], uv64[:, reg])
        for b, m in enumerate(models):
            referr[m] = max(referr.get(m, 0.0), float(e_ref[b].max()))
            worst_px[m] = max(worst_px.get(m, 0.0), float(np.abs(uv64[b, reg]).max()))
            # the reference's own masks are the fp64 restatement's on every regular point (Pinhole inverted, Spherical none)
            assert np.array_equal(ref_mask[b].reshape(-1)[reg], class_mask(m, in64[b])[reg]), (name, b)
            assert np.array_equal(in32[b, reg], in64[b, reg]), (name, b)
        lines.append(f"{name:28s} reference error {e_ref.max():.3e}  fp32 restatement error {e_r32.max():.3e}  regular points {n_reg} of {H * W}")
        out[name + ".xyz"], out[name + ".params"], out[name + ".models"] = xyz, params, np.asarray(models, dtype=np.int32)
        out[name + ".uv"], out[name + ".mask"], out[name + ".n_regular"] = ref_uv, ref_mask, np.int32(n_reg)
    for m, e in sorted(referr.items()):
        out["referr." + MODEL_NAMES[m]] = np.float64(e)
        px = bar(e) * max(worst_px[m], 1.0)
        lines.append(f"referr.{MODEL_NAMES[m]:11s} {e:.3e}   bar {bar(e):.3e}   = {px:.3e} px at the largest |uv| {worst_px[m]:.1f}  (margin {MARGIN:g} px)")
        worst_px[m] = px
    print("\n".join(lines))
    assert MARGIN >= 8 * max(worst_px.values()), f"margin {MARGIN} px below 8 x the largest bar in pixels {max(worst_px.values()):.3e}"
    rt = roundtrip_cases()
    lines.append("round-trip cases (every pixel valid): " + ", ".join(sorted(rt)))
    out["roundtrip"] = np.asarray(sorted(rt))
    print(lines[-1])
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    with open(BARS_TXT, "w") as f:
        f.write("tools/make_golden_camera_project.py: the reference's own fp32 Camera.project against the fp64 restatement, regular points\n")
        f.write("\n".join(lines) + "\n")
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
