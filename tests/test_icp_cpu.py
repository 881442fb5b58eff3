"""track_camera without a GPU (unidepth_amd/icp.py, include/unidepth_hip.h UdIcp): the functions of csrc/icp_point.h compiled for the host
and run under the host sanitizers (tests/icp_host/icp_host.cpp, a stand-alone program) -- ud_icp_row against the program's own chain of
the unchanged per-point functions and against the numpy restatement, bit for bit, for each closed-form frame model against each of the six
model cameras, the points form, shared and per-image T, mask, weights and normals on and off, both scenes, the edge shapes and the special
values; the sums against numpy's within the bound of two summation orders; ud_icp_solve and the whole loop against the restatement, bit
for bit; both known answers; the C-ABI's descriptor, every refusal of the entry points and the Python argument errors.  Shared helpers:
tests/icp_common.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import icp_common as ic

ROOT = ic.ROOT
F = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory)


def _options(c, mask, weights, normals):
    kw = {}
    if mask:
        kw["mask"] = c["mask"]
    if weights:
        kw["weights"] = c["weights"]
    if normals:
        kw["normals"], kw["cos_tol"] = c["normals"], c["cos_tol"]
    return kw


def _run_case(host, c, points=False, **kw):
    frame = dict(points=c["points"]) if points else dict(depth=c["depth"], params=c["params"], models_frame=c["models_frame"])
    return ic.host_run(host, mp=c["mp"], mn=c["mn"], mv=c["mv"], params_model=c["params_model"], models_model=c["models_model"], T=c["T"],
                       dist_tol=c["dist_tol"], **frame, **kw)


def _restated(c, r, points=False, mask=None, weights=None, normals=None, cos_tol=None):
    """the restatement image by image, fed the chain's points and coordinates where the camera is not a Pinhole -> the list of
    (matched, residual, rows, w)"""
    out = []
    for b in range(c["B"]):
        if points:
            P, live = c["points"][b], ic.finite(c["points"][b]).all(axis=0)
        else:
            P = ic.pinhole_points(c["depth"][b], c["params"][b]) if c["models_frame"][b] == ic.PINHOLE else r["p"][b]
            with np.errstate(all="ignore"):
                live = c["depth"][b] > 0
        if mask is not None:
            live = live & (mask[b] != 0)
        T = c["T"][b if len(c["T"]) > 1 else 0]
        uv = None if c["models_model"][b] == ic.PINHOLE else r["uv"][b]
        out.append(ic.restate_rows(P, live, T, c["models_model"][b], c["params_model"][b], c["mp"][b], c["mn"][b], c["mv"][b], c["dist_tol"], uv=uv,
                                   normals=None if normals is None else normals[b], cos_tol=cos_tol, weights=None if weights is None else weights[b]))
    return out


def _assert_rows(r, want, what):
    for b, (matched, res, g, _) in enumerate(want):
        assert np.array_equal(r["matched"][b], matched), (what, b, int((r["matched"][b] != matched).sum()))
        assert ic.same_bits(r["residual"][b], res) and ic.same_bits(r["rows"][b], g), (what, b)
        off = ~r["matched"][b]
        assert not r["residual"][b][off].view(np.uint32).any() and not r["rows"][b][:, off].view(np.uint32).any(), (what, b)


def _assert_system(r, want, what):
    """the program's sums in pixel order: bit-equal to the restatement's running sums, within the bound of numpy's own order, count exact"""
    for b, (matched, res, g, w) in enumerate(want):
        t = ic.terms(matched, res, g, w)
        S = r["systems"][0, b]
        assert ic.same_bits(S, ic.system(t, serial=True)), (what, b)
        assert (np.abs(S - ic.system(t, serial=False)) <= ic.system_bound(t)).all(), (what, b)
        assert S[29] == matched.sum() and S[30] == 0 and S[31] == 0, (what, b)


# ---- ud_icp_row ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame_model", ic.CLOSED, ids=[ic.NAMES[m] for m in ic.CLOSED])
def test_host_rows_for_every_model_pair(host, frame_model):
    """a frame of one closed-form model against a batch of all six model cameras, 29x41 against 37x53; shared and per-image T; mask,
    weights and normals + cos_tol each on and off.  The program exits non-zero when the fused function and its chain differ in one bit or a
    sanitizer reports; the restatement agrees bit for bit; every gate decides both ways in every image."""
    plain = None
    for per_image in (False, True):
        c = ic.mixed_case((frame_model,) * 6, ic.MODELS, per_image=per_image)
        for mask, weights, normals in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            kw = _options(c, mask, weights, normals)
            r = _run_case(host, c, **kw)
            want = _restated(c, r, **kw)
            what = (ic.NAMES[frame_model], per_image, mask, weights, normals)
            _assert_rows(r, want, what)
            _assert_system(r, want, what)
            share = r["matched"].reshape(6, -1).mean(axis=1)
            assert (share > 0.05).all() and (share < 0.95).all(), (what, share)
            if plain is None:
                plain = r["matched"]
            elif not per_image:
                assert (r["matched"] != plain).any() and not (r["matched"] & ~plain).any(), what      # the optional inputs are read


def test_host_points_form_and_edge_shapes(host):
    """the points form (the route of OPENCV / Fisheye624 frames: any point map), and 1x1, 2x3 and 1x257 frames against 1x1 and 2x3 model
    maps: fused equals chain equals restatement, the sanitizers are silent"""
    c = ic.mixed_case((ic.PINHOLE,) * 6, ic.MODELS)
    c["points"] = np.stack([ic.pinhole_points(c["depth"][b], c["params"][b]) for b in range(6)])
    c["points"][0, :, 0, :5] = [[np.nan, np.inf, 0, 1, 2]] * 3
    for kw in ({}, _options(c, 1, 1, 1)):
        r = _run_case(host, c, points=True, **kw)
        want = _restated(c, r, points=True, **kw)
        _assert_rows(r, want, "points")
        _assert_system(r, want, "points")
        assert 0.05 < r["matched"].mean() < 0.95
    hits = 0
    for (H, W), (Hm, Wm) in itertools.product(((1, 1), (2, 3), (1, 257)), ((1, 1), (2, 3))):
        c = ic.mixed_case((ic.PINHOLE, ic.EUCM, ic.MEI), (ic.PINHOLE, ic.OPENCV, ic.SPHERICAL), H=H, W=W, Hm=Hm, Wm=Wm)
        r = _run_case(host, c, **_options(c, 1, 1, 0))
        _assert_rows(r, _restated(c, r, **_options(c, 1, 1, 0)), (H, W, Hm, Wm))
        hits += int(r["matched"].sum())
    assert hits > 0


@pytest.mark.parametrize("name", [f"corner_{k}" for k in ic.CORNER_SIZES] + [f"smooth_{k}" for k in ic.SMOOTH_SIZES])
def test_host_scenes_rows_and_system(host, name):
    kind, key = name.split("_", 1)
    s = ic.corner(key) if kind == "corner" else ic.smooth(key)
    r = ic.host_scene(host, s)
    c = dict(B=1, depth=s["depth"][None], params=s["row"][None], models_frame=[ic.PINHOLE], T=s["T0"][None], models_model=[ic.PINHOLE],
             params_model=s["row_model"][None], mp=s["mp"][None], mn=s["mn"][None], mv=s["mv"][None], dist_tol=s["dist_tol"])
    want = _restated(c, r)
    _assert_rows(r, want, name)
    _assert_system(r, want, name)


def test_host_special_values(host):
    """NaN, +-inf, 0, -0.0 and negative values in the depth, the weights and T; NaN normals and infinite points in the model maps; model
    maps all invalid; every point behind the model camera: fused equals chain equals restatement, every comparison is false for a NaN and
    every unmatched output is exactly 0"""
    c = ic.special_case()
    kw = _options(c, 1, 1, 1)
    r = _run_case(host, c, **kw)
    _assert_rows(r, _restated(c, r, **kw), "special")
    m = r["matched"]
    assert not m[0].reshape(-1)[:6].any() and not m[0].reshape(-1)[8:13].any()          # the planted depths and weights (1e38, 1e-38, 1e-30 may match)
    assert not m[2].any() and not m[3].any() and not m[4].any() and m[0].any() and m[1].any()
    assert np.isfinite(r["residual"]).all() and np.isfinite(r["rows"]).all() and np.isfinite(r["systems"]).all()
    assert (r["systems"][0, 2:, :30] == 0).all()


# ---- ud_icp_solve ----------------------------------------------------------------------------------------------------------------------

def _scene_systems(host):
    S, T = [], []
    for s in [ic.corner(k) for k in ic.CORNER_SIZES] + [ic.smooth(k) for k in ic.SMOOTH_SIZES]:
        S.append(ic.host_scene(host, s)["systems"][0, 0])
        T.append(s["T0"])
    return np.stack(S), np.stack(T)


def _assert_solve(host, S, T, **kw):
    Tn, x, status = ic.host_solve(host, S, T, **kw)
    for b in range(len(S)):
        wT, wx, ws = ic.solve(S[b], T[b], **kw)
        assert status[b] == ws and ic.same_bits(x[b], wx) and ic.same_bits(Tn[b], wT), (b, kw, status[b], ws, x[b], wx)
    return Tn, x, status


def test_host_solve_equals_restatement(host):
    S, T = _scene_systems(host)
    Tn, x, status = _assert_solve(host, S, T)
    assert status.all() and (np.abs(x).max(axis=1) > 1e-3).all()
    A = np.zeros((len(S), 6, 6))
    for k, (i, j) in enumerate(ic.TRI):
        A[:, i, j] = A[:, j, i] = S[:, k]
    cond = np.linalg.cond(A)
    assert (cond[:4] > 30).all() and (cond[:4] < 70).all() and (cond[4:] > 1e3).all() and (cond[4:] < 1e4).all(), cond
    assert np.abs(np.einsum("bij,bj->bi", A, x) - S[:, 21:27]).max() <= 1e-9 * np.abs(S[:, 21:27]).max()
    # with damping: another answer, the same bits on both sides
    _, xd, sd = _assert_solve(host, S, T, damping=5.0)
    assert sd.all() and (np.abs(xd) < np.abs(x).max(axis=1, keepdims=True)).all() and not np.array_equal(xd, x)
    # count below min_count: status 0, x = 0, T untouched
    Tn, x0, s0 = _assert_solve(host, S, T, min_count=10 ** 6)
    assert not s0.any() and not x0.any() and ic.same_bits(Tn, T)
    # a NaN entry, in A and in b
    for slot in (0, 7, 20, 21, 26):
        Sn = S.copy()
        Sn[:, slot] = np.nan
        Tn, x0, s0 = _assert_solve(host, Sn, T)
        assert not s0.any() and not x0.any() and ic.same_bits(Tn, T), slot


def test_host_solve_singular_system(host):
    """a single fronto-parallel plane constrains three of the six freedoms: a pivot is not > 0, status 0, T untouched; damping makes it
    solvable"""
    H, W, f = 24, 32, 30.0
    row = ic.pinhole_row(H, W, f)
    depth = np.full((H, W), 2.0, F)
    mp = ic.pinhole_points(np.full((H, W), 2.125, F), row)
    mn = np.zeros((3, H, W), F)
    mn[2] = -1
    s = dict(depth=depth, row=row, row_model=row, mp=mp, mn=mn, mv=np.ones((H, W), np.uint8), T0=np.eye(4, dtype=F)[:3], dist_tol=0.5)
    r = ic.host_scene(host, s, iters=1)
    assert r["matched"].all() and r["status"][0, 0] == 0 and not r["x"].any() and ic.same_bits(r["Ts"][0, 0], s["T0"])
    S = r["systems"][0]
    _assert_solve(host, S, s["T0"][None])
    Tn, x, status = _assert_solve(host, S, s["T0"][None], damping=1e-3)
    # r = n . (m - q) = -0.125 with n = -z, and g . x = n . v: v_z = +0.125 moves q onto the model
    assert status[0] == 1 and abs(x[0, 5] - 0.125) < 1e-3 and np.abs(x[0, :5]).max() < 1e-6
    assert abs(Tn[0, 2, 3] - 0.125) < 1e-3


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------

CORNER_MEASURED, SMOOTH_FLOOR = ic.CORNER_MEASURED, ic.SMOOTH_FLOOR


@pytest.mark.parametrize("name", list(ic.CORNER_SIZES))
def test_host_loop_corner(host, name):
    """the host program's loop against the restated loop, bit for bit in every step's system, x, status and T; the known answer.
    Measured with the restatement after 8 iterations (rotation error in degrees, translation error): 48x64 0.0220, 1.81e-4; 24x32 0.0845,
    5.03e-3; 37x53 0.0658, 2.68e-3; 29x41 against 37x53 0.1260, 5.08e-3 -- the floor of nearest-pixel matches across the creases.  Matched
    share of the live pixels 84.4 % .. 92.7 % over all steps and sizes; cond(A) 40 .. 45.  Bars: 0.25 degrees and 0.01."""
    s = ic.corner(name)
    T, steps = ic.restated_track(s, 8)
    r = ic.host_scene(host, s, iters=8)
    for k, st in enumerate(steps):
        assert ic.same_bits(r["systems"][k, 0], st["S"]) and ic.same_bits(r["x"][k, 0], st["x"]) and r["status"][k, 0] == st["status"] == 1, k
        assert ic.same_bits(r["Ts"][k, 0], st["T"]), k
        assert 0.5 <= st["share"] <= 0.95, (k, st["share"])
    live = int((s["depth"] > 0).sum())
    assert 1 - steps[-1]["matched"] / live >= 0.02
    rot, tr = ic.pose_errors(r["Ts"][-1, 0], s["truth"])
    print(name, rot, tr)
    assert rot <= CORNER_MEASURED[name][0] and tr <= CORNER_MEASURED[name][1], (rot, tr)
    assert rot <= ic.CORNER_BARS[0] and tr <= ic.CORNER_BARS[1]
    rot0, tr0 = ic.pose_errors(s["T0"], s["truth"])
    assert abs(rot0 - 3.08) < 0.01 and abs(tr0 - 0.0707) < 1e-4


@pytest.mark.parametrize("name", list(ic.SMOOTH_SIZES))
def test_host_loop_smooth(host, name):
    """the smooth surface from its start: quadratic convergence to the identity, then the floor of fp32 rows.  Measured with the
    restatement: rotation error below 1e-3 degrees after 2 iterations; over iterations 3 .. 6 and the three sizes at most 5.6e-5 degrees
    and 8.2e-7 (SMOOTH_FLOOR).  The bar after 6 iterations is 8 times that.  Matched share 69.8 % .. 92.8 %."""
    s = ic.smooth(name)
    T, steps = ic.restated_track(s, 6)
    r = ic.host_scene(host, s, iters=6)
    for k, st in enumerate(steps):
        assert ic.same_bits(r["Ts"][k, 0], st["T"]) and ic.same_bits(r["systems"][k, 0], st["S"]) and r["status"][k, 0] == 1, k
        assert 0.5 <= st["share"] <= 0.95, (k, st["share"])
        if k >= 2:
            rot, tr = ic.pose_errors(st["T"], s["truth"])
            assert rot <= SMOOTH_FLOOR[0] and tr <= SMOOTH_FLOOR[1], (k, rot, tr)
    assert ic.pose_errors(steps[1]["T"], s["truth"])[0] < 1e-3
    rot, tr = ic.pose_errors(r["Ts"][-1, 0], s["truth"])
    assert rot <= 8 * SMOOTH_FLOOR[0] and tr <= 8 * SMOOTH_FLOOR[1]


def test_host_loop_keeps_rotations_orthogonal(host):
    """16 iterations, each rounding the nine entries of R to fp32 once (at most about 3.6e-7 per step): |R^T R - I|max <= 1e-5"""
    for s in (ic.corner("37x53"), ic.smooth("37x53")):
        r = ic.host_scene(host, s, iters=16)
        R = r["Ts"][-1, 0, :, :3].astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-5


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_icp_workspace_size_and_build_flags():
    from unidepth_amd import _lib
    wb = _lib.lib.ud_icp_workspace_bytes
    # 32 doubles per workgroup, sized for the most workgroups UdIcp.blocks may ask for: min(ceil(H * W / 256), 1024) per image
    assert wb(1, 1, 1) == 256 and wb(3, 1, 257) == 3 * 2 * 256 and wb(2, 256, 256) == 2 * 256 * 256 and wb(1, 518, 518) == 1024 * 256
    assert wb(1, 1, ic.SPAN + 1) == 257 * 256 and wb(1, 1, ic.SPAN - 256) == 255 * 256 and wb(2, 1024, 256) == 2 * 1024 * 256
    assert wb(0, 1, 1) == -1 and wb(257, 1, 1) == -1 and wb(1, 0, 1) == -1 and wb(1, 1 << 16, 1 << 15) == -1
    build = open(os.path.join(ROOT, "unidepth_amd", "csrc", "build.sh")).read()
    assert re.search(r"-ffp-contract=off [^\n]*-c icp\.hip", build)


def test_every_refusal():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_icp_linearize(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    assert lib.ud_icp_update(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    nan32, inf32, neg32 = ic.f32_bits(float("nan")), ic.f32_bits(float("inf")), ic.f32_bits(-0.5)
    nan64, inf64, neg64 = ic.f64_bits(float("nan")), ic.f64_bits(float("inf")), ic.f64_bits(-1e-300)

    def call(fn=lib.ud_icp_linearize, **kw):
        d = _lib.UdIcp()
        base = dict(depth=16, points=None, params=16, mask=None, weights=None, normals=None, model_points=16, model_normals=16, model_valid=16,
                    params_model=16, T=16, work=16, system=16, work_bytes=2 * 256, B=2, H=4, W=6, Hm=5, Wm=7, nT=1, solve=0, min_count=6, has_cos=0,
                    dist_tol_bits=ic.f32_bits(0.1), cos_tol_bits=0, damping_bits=0, stats_stride=0, blocks=0)
        base.update(kw)
        mf, mm = base.pop("mf", (1, 6)), base.pop("mm", (4, 5))
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(mf):
            d.model_frame[b] = m
        for b, m in enumerate(mm):
            d.model_model[b] = m
        return fn(C.byref(d), None), lib.ud_last_error().decode()
    solve = dict(solve=1, nT=2)
    for kw, msg in (
            (dict(B=0), "bad sizes"), (dict(B=-1), "bad sizes"), (dict(B=257), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-1), "bad sizes"),
            (dict(Hm=0), "bad sizes"), (dict(Wm=-2), "bad sizes"), (dict(H=1 << 15, W=1 << 14), "too large"), (dict(Hm=1 << 15, Wm=1 << 15), "too large"),
            (dict(depth=None), "exactly one"), (dict(points=16), "exactly one"), (dict(params=None), "null pointer"),
            (dict(model_points=None), "null pointer"), (dict(model_normals=None), "null pointer"), (dict(model_valid=None), "null pointer"),
            (dict(params_model=None), "null pointer"), (dict(T=None), "null pointer"), (dict(work=None), "null pointer"), (dict(system=None), "null pointer"),
            (dict(nT=0), "nT"), (dict(nT=3), "nT"),
            (dict(dist_tol_bits=nan32), "dist_tol"), (dict(dist_tol_bits=inf32), "dist_tol"), (dict(dist_tol_bits=neg32), "dist_tol"),
            (dict(has_cos=1, normals=16, cos_tol_bits=nan32), "cos_tol"), (dict(has_cos=1, normals=16, cos_tol_bits=ic.f32_bits(1.5)), "cos_tol"),
            (dict(has_cos=1, normals=16, cos_tol_bits=ic.f32_bits(-1.01)), "cos_tol"), (dict(has_cos=1, cos_tol_bits=0), "normals"),
            (dict(work_bytes=2 * 256 - 1), "workspace"), (dict(work_bytes=0), "workspace"), (dict(H=1, W=257, work_bytes=3 * 256), "workspace"),
            (dict(blocks=-1), "blocks"), (dict(blocks=1025), "blocks"),
            (dict(solve=1), "nT = B"), (dict(damping_bits=nan64, **solve), "damping"), (dict(damping_bits=inf64, **solve), "damping"),
            (dict(damping_bits=neg64, **solve), "damping"), (dict(min_count=-1, **solve), "min_count"), (dict(stats=16, stats_stride=3, **solve), "stats_stride"),
            (dict(mf=(0, 1)), "model tag"), (dict(mf=(1, 7)), "model tag"), (dict(mm=(0, 1)), "model tag"), (dict(mm=(1, 9)), "model tag"),
            (dict(mf=(4, 1)), "iterative frame model"), (dict(mf=(1, 5)), "iterative frame model")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    for kw, msg in ((dict(B=0), "bad sizes"), (dict(B=257), "bad sizes"), (dict(system=None), "null pointer"), (dict(T=None), "null pointer"),
                    (dict(nT=1), "nT = B"), (dict(damping_bits=nan64), "damping"), (dict(damping_bits=neg64), "damping"), (dict(min_count=-1), "min_count"),
                    (dict(stats=16, stats_stride=0), "stats_stride")):
        rc, err = call(lib.ud_icp_update, **{**solve, **kw})
        assert rc == -1 and msg in err and "ud_icp_update" in err, (kw, rc, err)
    # (nothing else can be called here: a descriptor that passes every check would be launched)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, icp
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    depth, mp, mn, mv, T = torch.rand(2, 1, 4, 6) + 1, torch.rand(2, 3, 5, 7), torch.rand(2, 3, 5, 7), torch.ones(2, 1, 5, 7, dtype=torch.bool), torch.eye(4)
    lin = [(f, lambda f, *a, **k: f(*a, **k)) for f in (icp.icp_linearize, icp.icp_linearize_composition)]
    trk = [(f, lambda f, *a, **k: f(*a, **k)) for f in (icp.track_camera, icp.track_camera_composition)]
    for f, run in lin + trk:
        fn = f.__name__
        ok = dict(dist_tol=0.1)
        for bad in (torch.rand(2, 2, 4, 6), torch.rand(4, 6), torch.ones(2, 1, 4, 6, dtype=torch.int64), torch.rand(0, 1, 4, 6), "depth"):
            with pytest.raises(ValueError, match=f"{fn}: frame"):
                run(f, bad, K, mp, mn, mv, K, T, **ok)
        with pytest.raises(ValueError, match=f"{fn}: camera is required"):
            run(f, depth, None, mp, mn, mv, K, T, **ok)
        with pytest.raises(ValueError, match=f"{fn}: camera of 3 images"):
            run(f, depth, K.expand(3, 3, 3), mp, mn, mv, K, T, **ok)
        with pytest.raises(ValueError, match=f"{fn}: at most"):
            run(f, torch.rand(257, 1, 1, 1), K, torch.rand(257, 3, 1, 1), torch.rand(257, 3, 1, 1), torch.ones(257, 1, 1, 1, dtype=torch.bool), K, T, **ok)
        for bad in (torch.rand(2, 2, 5, 7), torch.rand(3, 3, 5, 7), torch.rand(2, 3, 0, 7), torch.ones(2, 3, 5, 7, dtype=torch.int32), None):
            with pytest.raises(ValueError, match=f"{fn}: model_points"):
                run(f, depth, K, bad, mn, mv, K, T, **ok)
        for bad in (torch.rand(2, 3, 5, 6), torch.rand(1, 3, 5, 7), torch.ones(2, 3, 5, 7, dtype=torch.int32), None):
            with pytest.raises(ValueError, match=f"{fn}: model_normals"):
                run(f, depth, K, mp, bad, mv, K, T, **ok)
        for bad in (torch.ones(2, 1, 5, 6, dtype=torch.bool), torch.ones(2, 5, 7), torch.ones(1, 5, 7, dtype=torch.bool), None):
            with pytest.raises(ValueError, match=f"{fn}: model_valid"):
                run(f, depth, K, mp, mn, bad, K, T, **ok)
        with pytest.raises(ValueError, match=f"{fn}: model_camera"):
            run(f, depth, K, mp, mn, mv, None, T, **ok)
        with pytest.raises(ValueError, match=f"{fn}: model_camera of 3 images"):
            run(f, depth, K, mp, mn, mv, K.expand(3, 3, 3), T, **ok)
        for bad in (torch.eye(3), torch.eye(4).repeat(3, 1, 1), torch.eye(4).double(), "T"):
            with pytest.raises(ValueError, match=f"{fn}: transform"):
                run(f, depth, K, mp, mn, mv, K, bad, **ok)
        for bad in (-0.1, float("nan"), float("inf"), 1e300, "tol", None, True):
            with pytest.raises(ValueError, match=f"{fn}: dist_tol"):
                run(f, depth, K, mp, mn, mv, K, T, dist_tol=bad)
        nf = torch.rand(2, 3, 4, 6)
        for bad in (-1.5, 1.01, float("nan"), "c", True):
            with pytest.raises(ValueError, match=f"{fn}: cos_tol"):
                run(f, depth, K, mp, mn, mv, K, T, cos_tol=bad, normals=nf, **ok)
        with pytest.raises(ValueError, match=f"{fn}: cos_tol needs"):
            run(f, depth, K, mp, mn, mv, K, T, cos_tol=0.5, **ok)
        for bad in (torch.rand(2, 3, 4, 5), torch.rand(1, 3, 4, 6), torch.ones(2, 3, 4, 6, dtype=torch.int32), "n"):
            with pytest.raises(ValueError, match=f"{fn}: normals"):
                run(f, depth, K, mp, mn, mv, K, T, normals=bad, **ok)
        for bad in (torch.ones(2, 1, 4, 5, dtype=torch.bool), torch.ones(2, 4, 6), torch.ones(1, 4, 6, dtype=torch.bool), "m"):
            with pytest.raises(ValueError, match=f"{fn}: mask"):
                run(f, depth, K, mp, mn, mv, K, T, mask=bad, **ok)
        for bad in (torch.ones(2, 1, 4, 5), torch.ones(2, 4, 6, dtype=torch.bool), torch.ones(1, 4, 6), "w"):
            with pytest.raises(ValueError, match=f"{fn}: weights"):
                run(f, depth, K, mp, mn, mv, K, T, weights=bad, **ok)
        # well-formed arguments on the CPU: the HIP kernels are the only implementation
        eucm = cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))
        opencv = cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12))
        for args, kw in (((depth, K, mp, mn, mv, K, T), {}), ((depth[:, 0].double(), eucm, mp, mn, mv[:, 0].to(torch.uint8), opencv, T[:3].expand(2, 3, 4)), {}),
                         ((torch.rand(2, 3, 4, 6), None, mp, mn, mv, eucm, T), dict(cos_tol=0.5, normals=nf, mask=torch.ones(2, 4, 6, dtype=torch.bool),
                                                                                  weights=torch.ones(2, 1, 4, 6)))):
            with pytest.raises(RuntimeError, match="GPU"):
                run(f, *args, **ok, **kw)
    for f in (icp.icp_linearize, icp.icp_linearize_composition):
        with pytest.raises(ValueError, match=f"{f.__name__}: transform"):
            f(depth, K, mp, mn, mv, K, None, dist_tol=0.1)
    for f in (icp.track_camera, icp.track_camera_composition):
        for bad in (0, -1, 1001, 2.0, True, None):
            with pytest.raises(ValueError, match=f"{f.__name__}: iters"):
                f(depth, K, mp, mn, mv, K, iters=bad, dist_tol=0.1)
        for bad in (-1.0, float("nan"), float("inf"), "d", True):
            with pytest.raises(ValueError, match=f"{f.__name__}: damping"):
                f(depth, K, mp, mn, mv, K, damping=bad, dist_tol=0.1)
        for bad in (-1, 1.0, True, None, 2 ** 31):
            with pytest.raises(ValueError, match=f"{f.__name__}: min_count"):
                f(depth, K, mp, mn, mv, K, min_count=bad, dist_tol=0.1)
        with pytest.raises(RuntimeError, match="GPU"):
            f(depth, K, mp, mn, mv, K, dist_tol=0.1)                                      # transform=None: the identity
    S = torch.zeros(2, 32, dtype=torch.float64)
    for bad in (torch.zeros(2, 32), torch.zeros(2, 30, dtype=torch.float64), torch.zeros(32, dtype=torch.float64), torch.zeros(0, 32, dtype=torch.float64), "S"):
        with pytest.raises(ValueError, match="icp_solve: system"):
            icp.icp_solve(bad, T)
    for bad in (None, torch.eye(3), torch.eye(4).repeat(3, 1, 1), torch.eye(4).double()):
        with pytest.raises(ValueError, match="icp_solve: transform"):
            icp.icp_solve(S, bad)
    with pytest.raises(ValueError, match="icp_solve: damping"):
        icp.icp_solve(S, T, damping=-1.0)
    with pytest.raises(ValueError, match="icp_solve: min_count"):
        icp.icp_solve(S, T, min_count=-1)
    with pytest.raises(ValueError, match="icp_solve: at most"):
        icp.icp_solve(torch.zeros(257, 32, dtype=torch.float64), T)
    with pytest.raises(RuntimeError, match="GPU"):
        icp.icp_solve(S, T)
    for name in ("icp_linearize", "icp_linearize_composition", "icp_solve", "track_camera", "track_camera_composition"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(icp, name)
    assert hasattr(unidepth_amd.TsdfVolume, "track")
    doc = " ".join(unidepth_amd.TsdfVolume.track.__doc__.split())
    assert "VOLUME (world) TO CAMERA" in doc and "invert_rigid" in doc
    assert "FRAME CAMERA TO MODEL CAMERA" in " ".join(icp.track_camera.__doc__.split())
