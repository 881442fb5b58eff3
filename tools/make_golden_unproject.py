"""Golden vectors of unproject_camera (unidepth_amd/unproject.py, csrc/unproject.hip): the reference's own Camera.unproject
(unidepth/utils/camera.py, torch on the CPU) at seeded image coordinates -> tests/golden/unproject.npz.

    python tools/make_golden_unproject.py          (needs the reference tree; only its outputs, masks, iteration counts, the camera rows,
                                                    a checksum of the seeded inputs and measured errors are written)

This module also holds what the tests share: CASES / case_inputs(name) (the cameras of tools/make_golden_gt_points.py's cases with a
seeded coordinate set each, uniform draws only, the same bits on every machine) and an independent numpy restatement of
ud_camera_unproject (include/unidepth_hip.h UdCameraUnproject): unproject(..., dtype=np.float32) rounds every operation separately in
fp32 -- the kernel's definition -- and unproject(..., dtype=np.float64) is the same expression in fp64, the value errors are measured
from.  It covers the masks and the normalize and depth forms.  Nothing from the reference is imported at module import time.

The coordinate set of an image has N = H * W points (so it can be passed planar, [B,2,H,W], as the reference wants it, or as rows):
REGULAR points first, uniform inside the image and off the integer grid; then N_OUTSIDE points up to half the image's size outside it;
the last one is a NaN coordinate for the closed-form models and MEI.  An OPENCV / Fisheye624 image has an in-image point there instead:
a NaN would keep its radial loop running to the end, so the NaN coordinate of those models has cases of its own (NAN_CASES, "<case>+nan").
The depths (for the depth form and the round trip) are uniform in [0.2, 20] with 0, a negative, a value below 1e-4 and a NaN on the
outside points.

The early exit of the OPENCV / Fisheye624 radial loop compares the maximum over the coordinate set with 1e-3.  case_inputs() settles
every such camera over ITS coordinate set as make_golden_gt_points.settle() does over the grid: the radial coefficients are scaled in
small steps until the fp32 restatement's largest |residual| lies outside [0.5e-3, 2e-3] at every iteration.  main() asserts that the
reference takes the restatement's number of iterations for every camera, calling it one camera at a time with uv[b:b+1] (a multi-row
MEI broadcasts wrongly there).

Tolerances are measured: main() records per model the reference's own fp32 error against the fp64 restatement, |d| / max(|truth|, 1e-4)
per component ("referr.<Model>"); the kernel's bar is make_golden_gt_points.bar() = max(4 x that, 8 x 2^-24).  A second set,
"rterr.<Model>", is the reference's own round trip project(reconstruct-rule(unproject(uv), depth)) - uv on the regular points,
|d| / max(|uv|, 1); EUCM points outside the mask are exempt, and the draw keeps them under a tenth of an image's regular points."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "unproject.npz")

_spec = importlib.util.spec_from_file_location("make_golden_camera_project", os.path.join(ROOT, "tools", "make_golden_camera_project.py"))
cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cp)
gp = cp.gp

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = gp.PINHOLE, gp.EUCM, gp.SPHERICAL, gp.OPENCV, gp.FISHEYE624, gp.MEI
MODEL_NAMES, ITERATIVE, bar = gp.MODEL_NAMES, gp.ITERATIVE, gp.bar
N_OUTSIDE = 4
NAN_CASES = ("opencv_5x7_b2_tan", "fisheye624_9x29_b2")
CASES = tuple(gp.CASES) + tuple(n + "+nan" for n in NAN_CASES)
MASKED_SHARE = 0.10                                            # EUCM: regular points outside the mask, per image, stay below this


def base_case(name):
    return name[:-4] if name.endswith("+nan") else name


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _direction(m, p, u, v, dt, info, b):
    """(x, y, z, mask) of one camera before the output form: Pinhole before its division, EUCM's z before its clamp."""
    one, two = dt(1), dt(2)
    c = lambda val: dt(np.float32(val))
    ones = np.ones(u.shape, bool)
    if m == PINHOLE:
        x, y = (u - p[2]) / p[0], (v - p[3]) / p[1]
        # z: 1, or NaN when an intrinsic or a coordinate is not finite (the last row of K^-1 times (u, v, 1) in the reference)
        return x, y, ((dt(0) * (p[0] + p[1] + p[2] + p[3]) + dt(0) * u) + dt(0) * v) + one, ones
    if m == EUCM:
        al, be = p[4], p[5]
        mx, my = (u - p[2]) / p[0], (v - p[3]) / p[1]
        r2 = mx * mx + my * my
        sv = one - (two * al - one) * be * r2
        mz = (one - be * (al * al) * r2) / (al * np.sqrt(gp._floor(sv, c(1e-5))) + (one - al))
        cf = one / np.sqrt(mx * mx + my * my + mz * mz + c(1e-5))
        z = cf * mz
        lim = c(1e6) if al < c(0.5) else one / (be * (two * al - one))
        return cf * mx, cf * my, z, (r2 < lim) & (z > c(1e-3))
    if m == SPHERICAL:
        lon = (u - (p[4] - one) / two) / (p[4] - one) * (two * p[6])
        lat = (v - (p[5] - one) / two) / (p[5] - one) * (two * p[7])
        cl = np.cos(lat)
        x, y, z = cl * np.sin(lon), np.sin(lat), cl * np.cos(lon)
        n = gp._floor(np.sqrt(x * x + y * y + z * z), c(1e-5))
        return x / n, y / n, z / n, ones
    if m in ITERATIVE:
        dx, dy, maxima, st = gp._solve_radial(p, m, u, v, dt)
        if info is not None:
            info.setdefault("maxima", {})[b] = maxima
            info.setdefault("steps", {})[b] = st
        return dx, dy, np.ones_like(dx), ones
    if m == MEI:
        dx, dy, pz = gp._mei(p, u, v, dt)
        return dx, dy, pz, ones
    raise ValueError(f"model tag {m}")


def _form(m, x, y, z, d, normalize, dt):
    """ud_cam_unproject_form: what goes out for a direction, and the Pinhole mask."""
    c = lambda val: dt(np.float32(val))
    mask = np.ones(x.shape, bool)
    if m == PINHOLE:
        zc = gp._floor(z, c(1e-4))
        mask = z / zc > c(1e-4)
        if d is not None:
            dc = gp._floor(d, dt(0))
            return np.stack([x / zc * dc, y / zc * dc, z / zc * dc], axis=-1), mask
        x, y, z = x / zc, y / zc, z / zc
    elif m == EUCM:
        z = gp._floor(z, c(1e-3))
    if d is not None:
        if m == SPHERICAL:
            return np.stack([x * d, y * d, z * d], axis=-1), mask
        zc, dc = gp._floor(z, c(1e-4)), gp._floor(d, c(1e-4))
        return np.stack([x / zc * dc, y / zc * dc, z / zc * dc], axis=-1), mask
    if normalize:
        n = gp._floor(np.sqrt(x * x + y * y + z * z), c(1e-4))
        return np.stack([x / n, y / n, z / n], axis=-1), mask
    return np.stack([x, y, z], axis=-1), mask


def unproject(uv, params, models, dtype=np.float32, info=None, depth=None, normalize=False):
    """ud_camera_unproject: uv [B,N,2] (or [1,N,2], shared), params [B,16] (fp32 values), models [B], depth None / [B,N] -> (rays [B,N,3]
    in `dtype`, mask bool [B,N]), every operation rounded separately in `dtype`.  info (a dict) receives {"maxima": {b: [...]},
    "steps": {b: n}} of the iterative images, each over its own N points."""
    assert not (normalize and depth is not None)
    dt = np.dtype(dtype).type
    B = len(models)
    uv = np.asarray(uv, dtype=np.float32).astype(dtype)
    N = uv.shape[1]
    params = np.asarray(params, dtype=np.float32).reshape(B, 16).astype(dtype)
    depth = None if depth is None else np.asarray(depth, dtype=np.float32).reshape(B, N).astype(dtype)
    rays, mask = np.zeros((B, N, 3), dtype=dtype), np.zeros((B, N), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            src = uv[b if uv.shape[0] > 1 else 0]
            u, v = np.ascontiguousarray(src[:, 0]), np.ascontiguousarray(src[:, 1])
            m = int(models[b])
            x, y, z, mk = _direction(m, params[b], u, v, dt, info, b)
            rays[b], fm = _form(m, x, y, z, None if depth is None else depth[b], normalize, dt)
            mask[b] = mk & fm
    assert rays.dtype == dtype
    return rays, mask


def ray_error(delta, truth):
    """|delta| / max(|truth|, 1e-4) per component, fp64; NaN positions of the truth give 0 (they are compared separately)."""
    with np.errstate(invalid="ignore"):
        r = np.abs(delta.astype(np.float64)) / np.maximum(np.abs(truth.astype(np.float64)), 1e-4)
    return np.where(np.isnan(truth), 0.0, r)


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def rows(planar):
    """[B,C,H,W] -> [B,H*W,C]"""
    B, C = planar.shape[:2]
    return np.ascontiguousarray(planar.reshape(B, C, -1).transpose(0, 2, 1))


def planar(rws, H, W):
    """[B,N,C] -> [B,C,H,W]"""
    return np.ascontiguousarray(rws.transpose(0, 2, 1)).reshape(rws.shape[0], rws.shape[2], H, W)


def _settle(model, row, uv_sets):
    """the row with its radial coefficients scaled by (1 + 0.03 j), the smallest j at which the fp32 restatement's residual maximum over
    each of the coordinate sets (one per image the camera serves) avoids gp.MARGIN at every iteration"""
    for j in range(64):
        p = row.copy()
        p[4:10] = (row[4:10] * np.float32(1.0 + 0.03 * j)).astype(np.float32)
        info = {}
        unproject(uv_sets, np.repeat(p[None], len(uv_sets), axis=0), [model] * len(uv_sets), np.float32, info)
        if all(gp.margins_ok(info.get("maxima", {}).get(b, [])) for b in range(len(uv_sets))):
            return p
    raise AssertionError(f"no scaling of {row} keeps the residual maxima out of {gp.MARGIN}")


_CASE_CACHE = {}


def n_regular(name):
    H, W = gp.CASES[base_case(name)][:2]
    return H * W - N_OUTSIDE - 1


def case_inputs(name):
    """(uv fp32 [B,N,2], depth fp32 [B,N], params fp32 [B,16], models [B]) of a case, N = H * W: see the module docstring."""
    if name in _CASE_CACHE:
        return _CASE_CACHE[name]
    base = base_case(name)
    H, W = gp.CASES[base][:2]
    _, params, models = gp.case_rows(base)
    params = params.copy()
    B, N, n_reg = len(models), H * W, n_regular(name)
    g = torch.Generator().manual_seed(9100 + sorted(gp.CASES).index(base))
    size = np.array([W, H], dtype=np.float32)
    uv = np.zeros((B, N, 2), dtype=np.float32)
    for b in range(B):
        for _ in range(64):
            inside = torch.rand(N, 2, generator=g).numpy() * size
            if models[b] != EUCM:
                break
            _, mk = unproject(inside[None, :n_reg], params[b:b + 1], [EUCM], np.float64)
            if (~mk).mean() < 0.8 * MASKED_SHARE:
                break
        else:
            raise AssertionError(f"{name}: no draw keeps the masked share of image {b} under {MASKED_SHARE}")
        assert (inside != np.rint(inside)).all(), "a drawn coordinate sits on the integer grid"
        uv[b] = inside
        out = (2.0 * torch.rand(N_OUTSIDE, 2, generator=g).numpy() - 0.5) * size
        uv[b, n_reg:n_reg + N_OUTSIDE] = out.astype(np.float32)
        if name.endswith("+nan") or models[b] not in ITERATIVE:
            uv[b, N - 1] = (np.nan, 0.5 * H)
    depth = (0.2 + 19.8 * torch.rand(B, N, generator=g)).float().numpy()
    depth[:, n_reg], depth[:, n_reg + 1], depth[:, n_reg + 2], depth[0, n_reg + 3] = 0.0, -1.5, 5e-5, np.nan
    if len(gp.CASES[base][2]) == 1:                             # one camera for every image: one row, settled over all of them
        if models[0] in ITERATIVE:
            params[:] = _settle(models[0], params[0], uv)
    else:
        for b, m in enumerate(models):
            if m in ITERATIVE:
                params[b] = _settle(m, params[b], uv[b:b + 1])
    _CASE_CACHE[name] = (uv, depth, params, list(models))
    return _CASE_CACHE[name]


def checksum(a):
    return np.uint64(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_output(rc, name):
    """(rays fp32 [B,N,3], mask uint8 [B,N]: 0 / 1, or 2 where the class sets none, iterations of the radial loop per image or -1, round
    trip uv fp32 [B,N,2]) of a case from the reference's own unproject / project, one camera at a time"""
    uv, depth, params, models = case_inputs(name)
    H, W = gp.CASES[base_case(name)][:2]
    B, N = uv.shape[:2]
    grid, dmap = torch.from_numpy(planar(uv, H, W)), torch.from_numpy(depth.reshape(B, 1, H, W))
    outs, masks, steps, trips = [], [], [], []
    seen = []
    real_max = torch.max

    def counting_max(*a, **k):                                # the loop's `torch.max(torch.abs(residual))`: one call per look
        val = real_max(*a, **k)
        if isinstance(val, torch.Tensor) and val.ndim == 0:
            seen.append(float(val))
        return val

    for b, m in enumerate(models):
        cam = gp.make_camera(rc, m, params[b])
        del seen[:]
        torch.max = counting_max
        try:
            rays = cam.unproject(grid[b:b + 1])
        finally:
            torch.max = real_max
        assert rays.dtype == torch.float32 and tuple(rays.shape) == (1, 3, H, W), (name, b, rays.shape)
        mask = getattr(cam, "unprojection_mask", None)
        assert (mask is not None) == (m in (PINHOLE, EUCM)), (name, b)
        masks.append(np.full((1, N), 2, np.uint8) if mask is None else mask.numpy().astype(np.uint8).reshape(1, N))
        steps.append((len(seen) - 1 if seen and seen[-1] < 1e-3 else len(seen)) if m in ITERATIVE else -1)
        outs.append(rows(rays.numpy()))
        d = dmap[b:b + 1]
        if m == PINHOLE:
            pts = rays * d.clip(min=0.0)
        elif m == SPHERICAL:
            pts = rays * d
        else:
            pts = rays / rays[:, -1:].clamp(min=1e-4) * d.clamp(min=1e-4)
        trips.append(rows(gp.make_camera(rc, m, params[b]).project(pts).numpy()))
    return np.concatenate(outs), np.concatenate(masks), steps, np.concatenate(trips)


def class_mask(model, mask):
    """what the class's unprojection_mask is for a restated `mask`: 2 where the class sets none"""
    return mask.astype(np.uint8) if model in (PINHOLE, EUCM) else np.full(mask.shape, 2, np.uint8)


def main():
    rc = gp.reference_module()
    out, referr, rterr = {}, {}, {}
    for name in CASES:
        uv, depth, params, models = case_inputs(name)
        n_reg = n_regular(name)
        ref, ref_mask, ref_steps, trip = reference_output(rc, name)
        info = {}
        r32, m32 = unproject(uv, params, models, np.float32, info)
        truth, m64 = unproject(uv, params, models, np.float64)
        assert np.array_equal(np.isnan(ref), np.isnan(truth)) and np.array_equal(np.isnan(r32), np.isnan(truth)), name
        for b, m in enumerate(models):
            if m in ITERATIVE:
                assert gp.margins_ok(info.get("maxima", {}).get(b, [])), (name, b, info["maxima"][b])
                assert info.get("steps", {}).get(b, 0) == ref_steps[b], (name, b, info.get("steps"), ref_steps)
            assert np.array_equal(ref_mask[b], class_mask(m, m64[b])) and np.array_equal(m32[b], m64[b]), (name, b)
            if m == EUCM:
                assert (~m64[b, :n_reg]).mean() < MASKED_SHARE, (name, b)
        e_ref, e_r32 = ray_error(ref - truth, truth), ray_error(r32 - truth, truth)
        e_trip = cp.uv_error(trip[:, :n_reg] - uv[:, :n_reg], uv[:, :n_reg])
        assert np.isfinite(trip[:, :n_reg]).all(), name
        for b, m in enumerate(models):
            referr[m] = max(referr.get(m, 0.0), float(e_ref[b].max()))
            keep = m64[b, :n_reg] if m == EUCM else np.ones(n_reg, bool)
            rterr[m] = max(rterr.get(m, 0.0), float(e_trip[b][keep].max()))
        steps32 = [info.get("steps", {}).get(b, -1) for b in range(len(models))]
        print(f"{name:30s} reference error {e_ref.max():.3e}  fp32 restatement error {e_r32.max():.3e}  "
              f"restatement vs reference {ray_error(r32 - ref, truth).max():.3e}  iterations {steps32}")
        out[name + ".params"], out[name + ".models"] = params, np.asarray(models, dtype=np.int32)
        out[name + ".sum"] = np.asarray([checksum(uv), checksum(depth)], dtype=np.uint64)
        out[name + ".out"], out[name + ".mask"], out[name + ".steps"] = ref, ref_mask, np.asarray(ref_steps, dtype=np.int32)
    for m in sorted(referr):
        out["referr." + MODEL_NAMES[m]], out["rterr." + MODEL_NAMES[m]] = np.float64(referr[m]), np.float64(rterr[m])
        print(f"referr.{MODEL_NAMES[m]:11s} {referr[m]:.3e}   bar {bar(referr[m]):.3e}   round trip {rterr[m]:.3e}   bound {4 * rterr[m]:.3e}")
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")
    assert os.path.getsize(GOLDEN) <= os.path.getsize(gp.GOLDEN)


if __name__ == "__main__":
    main()
