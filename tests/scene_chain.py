"""What the two scene-truth modules share (not a test module): the figures -- every one an error of an op's output against
tests/scene_truth.py's analytic scene, in voxels, pixels or degrees -- the bars with the measurements they come from, and the chain run
through the host programs (tsdf_host, tsdf_render_host, tsdf_mesh_host, icp_host: the headers the kernels compile, built for the CPU).
The GPU module runs the same chain through the Python API and hands its outputs to the same figure functions.

A bar is 1.5 times the figure the correct chain gives (profiles/scene_truth.txt holds every measurement, CPU and MI355X, with the figure
each planted defect gives); a bar is kept only where a planted defect drives the figure to at least twice the bar."""
import numpy as np

import icp_common as ic
import scene_truth as st
import tsdf_common as tc
import tsdf_mesh_common as tm
import tsdf_render_common as tr

F = np.float32
CREASE_K = 2.0                                         # mesh vertices and cloud points are compared further than this many voxels from a crease


# What the correct chain measures against the analytic scene, magnitudes rounded up in the fourth digit: voxels, pixels (uv), degrees
# (angle, track's and the loops' first component) or shares.  The a, b, track and f rows and the two iterative models of e were
# measured on the MI355X through the Python API; c, d, the closed-form models of e and f4 through the host programs AND on the MI355X,
# with equal figures (profiles/scene_truth.txt).  Triples are (mean signed, mean absolute, maximum), pairs (mean, maximum), the pose
# rows (rotation error in degrees, translation error); f.*.worst is the largest over the frames (and over the run with cos_tol).
MEASURED = {
    "a.pinhole.points": (1.041e-06, 3.72e-06),
    "a.pinhole.angle": (0.01083, 0.7025),
    "a.eucm.points": (1.346e-06, 8.059e-06),
    "a.eucm.angle": (0.01038, 0.7096),
    "a.spherical.points": (1.823e-06, 8.023e-06),
    "a.spherical.angle": (0.01228, 0.6612),
    "a.opencv.points": (1.54e-06, 7.822e-06),
    "a.opencv.angle": (0.01082, 0.623),
    "a.fisheye624.points": (1.594e-06, 1.286e-05),
    "a.fisheye624.angle": (0.01285, 0.629),
    "a.mei.points": (1.898e-06, 1.501e-05),
    "a.mei.angle": (0.01042, 0.7312),
    "b.warp.eucm.uv": (2.994e-06, 1.218e-05),
    "b.warp.eucm.proj_depth": (1.225e-06, 4.888e-06),
    "b.warp.eucm.fetched": (0.003921, 0.003942, 0.04004),
    "b.warp.spherical.uv": (4.295e-06, 2.023e-05),
    "b.warp.spherical.proj_depth": (1.881e-06, 8.358e-06),
    "b.warp.spherical.fetched": (0.002663, 0.002663, 0.03472),
    "b.warp.opencv.uv": (3.4e-06, 1.449e-05),
    "b.warp.opencv.proj_depth": (1.225e-06, 4.888e-06),
    "b.warp.opencv.fetched": (0.003325, 0.003325, 0.03141),
    "b.warp.fisheye624.uv": (3.68e-06, 1.813e-05),
    "b.warp.fisheye624.proj_depth": (1.217e-06, 5.414e-06),
    "b.warp.fisheye624.fetched": (0.001425, 0.00152, 0.027),
    "b.consistency.closed.missed": (0.0,),
    "b.consistency.closed.count": (0.0,),
    "b.consistency.closed.fused": (0.003055,),
    "b.consistency.mixed.missed": (0.0,),
    "b.consistency.mixed.count": (0.0,),
    "b.consistency.mixed.fused": (0.003138,),
    "track.pinhole": (0.03743, 0.0006131),
    "track.eucm": (0.0246, 0.0002509),
    "track.spherical": (0.02169, 0.0002962),
    "track.opencv": (0.009891, 0.0006611),
    "track.fisheye624": (0.009606, 0.0004005),
    "track.mei": (0.02481, 0.0002712),
    "c.fusion": (0.001798, 0.04121, 0.3997),
    "c.sign": (0.003549,),
    "c.weight": (0.0,),
    "d.points": (0.008766, 0.03982, 1.079),
    "d.mesh": (0.01549, 0.02807, 0.848),
    "d.mesh.angle": (3.098, 50.42),
    "d.mesh.wound_wrong": (0.0,),
    "e.pinhole.3.depth": (0.01754, 0.02623, 0.3932),
    "e.pinhole.3.points": (0.03006, 0.4223),
    "e.pinhole.3.angle": (1.712, 26.6),
    "e.pinhole.3.invalid": (0.0001255,),
    "e.eucm.9.depth": (0.02091, 0.03222, 0.4263),
    "e.eucm.9.points": (0.03796, 0.4397),
    "e.eucm.9.angle": (2.224, 22.08),
    "e.eucm.9.invalid": (0.04695,),
    "e.spherical.3.depth": (0.02029, 0.02971, 0.5477),
    "e.spherical.3.points": (0.02971, 0.5477),
    "e.spherical.3.angle": (1.755, 22.92),
    "e.spherical.3.invalid": (0.001332,),
    "e.mei.9.depth": (0.02099, 0.03224, 0.4295),
    "e.mei.9.points": (0.03797, 0.4431),
    "e.mei.9.angle": (2.219, 22.1),
    "e.mei.9.invalid": (0.04792,),
    "e.opencv.3.depth": (0.01797, 0.02665, 0.3838),
    "e.opencv.3.points": (0.03078, 0.4074),
    "e.opencv.3.angle": (1.77, 23.63),
    "e.opencv.3.invalid": (0.0,),
    "e.fisheye624.9.depth": (0.02254, 0.03159, 0.7663),
    "e.fisheye624.9.points": (0.0355, 0.7869),
    "e.fisheye624.9.angle": (1.959, 26.75),
    "e.fisheye624.9.invalid": (0.001123,),
    "f.pinhole.worst": (0.3103, 0.01829),
    "f.pinhole.drift": (0.3103, 0.01829),
    "f.pinhole.mesh": (0.05723, 0.06618, 0.4851),
    "f.pinhole.mesh.angle": (2.954, 36.67),
    "f.pinhole.mesh.wound_wrong": (0.0,),
    "f.eucm.worst": (0.331, 0.01959),
    "f.eucm.drift": (0.331, 0.01959),
    "f.eucm.mesh": (0.06981, 0.07785, 0.5837),
    "f.eucm.mesh.angle": (3.635, 37.53),
    "f.eucm.mesh.wound_wrong": (0.0,),
    "f.mei.worst": (0.3374, 0.02009),
    "f.mei.drift": (0.3374, 0.02009),
    "f.mei.mesh": (0.07144, 0.0795, 0.5842),
    "f.mei.mesh.angle": (3.654, 37.03),
    "f.mei.mesh.wound_wrong": (0.0,),
    "f.batch.eucm.worst": (0.1875, 0.01089),
    "f4.pinhole.worst": (0.1892, 0.01373),
    "f4.pinhole.mesh": (0.03862, 0.05247, 0.7317),
    "f4.pinhole.mesh.angle": (3.949, 49.9),
    "f4.pinhole.mesh.wound_wrong": (0.0,),
}
# the share of a frame's live pixels the last ICP step matches: 0.629 .. 0.686 measured over the 12 frames of the three loops (the rest
# are the crease bands the prediction leaves invalid and the pixels beyond dist_tol); the lower bound is the smallest over 1.5
MATCHED_SHARE = (0.419, 1.0)


def _tuple(values):
    return tuple(float(v) for v in values) if isinstance(values, (tuple, list)) else (float(values),)


def line(name, values):
    """one line of profiles/scene_truth.txt"""
    return f"scene_truth: {name}: " + " ".join(f"{v:.4g}" for v in _tuple(values))


def within(name, values):
    """print the figure, then assert every component's magnitude within its bar: 1.5 times MEASURED[name]"""
    values = _tuple(values)
    print(line(name, values))
    assert name in MEASURED, f"{name}: no measurement to set a bar from"
    bars = tuple(1.5 * m for m in MEASURED[name])
    assert len(bars) == len(values), (name, len(bars), len(values))
    for k, (v, b) in enumerate(zip(values, bars)):
        assert abs(v) <= b, f"{name}[{k}]: {v:.4g} above the bar {b:.4g} (1.5 x the measured {MEASURED[name][k]:.4g})"


def exceeds(name, values, which, defect):
    """print the figure a planted defect gives, then assert that the components `which` reach at least TWICE their bars (and are not
    0 where the bar is 0): the proof that the bar bites"""
    values = _tuple(values)
    print(line(f"{name} [{defect}]", values))
    for k in which:
        b = 1.5 * MEASURED[name][k]
        assert abs(values[k]) >= 2 * b and abs(values[k]) > 0, f"{name}[{k}] with {defect}: {values[k]:.4g} below twice the bar {b:.4g}"


# ---- a. point maps and normals -------------------------------------------------------------------------------------------------------

def rotated_view(model, size=st.VIEW):
    """the view of section a: `model` from the trajectory's first pose (8.9 degrees from the middle one, about all three axes)"""
    H, W, f = size
    return st.view(model, st.row(model, H, W, f), H, W, st.trajectory()[0])


def map_figures(points, normals, truth):
    """gt_points' and normals_camera's maps [3,H,W] against the oracle's view over its smooth pixels: (mean, maximum) distance of the
    points in voxels, (mean, maximum) angle of the normals in degrees, the share of smooth pixels without a normal"""
    m = truth["smooth"]
    pe = np.linalg.norm(np.asarray(points, np.float64) - truth["points"], axis=0)[m] / st.VOXEL
    n = np.asarray(normals, np.float64)
    has = m & (n != 0).any(axis=0)
    a = st.angle_deg(n[:, has], truth["normals"][:, has])
    return dict(points=(float(pe.mean()), float(pe.max())), angle=(float(a.mean()), float(a.max())), no_normal=float(1 - has.sum() / m.sum()))


# ---- b. cross-view geometry ------------------------------------------------------------------------------------------------------------

# two camera centres near the reference's and two far to its side: far enough for the sphere to hide a tenth of the reference view from
# them (11 %), near enough for half of it to be seen by all four (53 %)
CROSS_EYES = ((-0.4, 0.0, 0.0), (1.9, -0.2, 0.4), (0.2, -0.5, 0.0), (1.4, 0.8, 0.4))
CROSS_TARGET = (0.3, 0.1, 2.6)
CROSS_ROLLS = (0.1, -0.15, 0.2, -0.1)
CROSS_CLOSED = (st.EUCM, st.SPHERICAL, st.MEI, st.PINHOLE)        # the fused kernel
CROSS_MIXED = (st.OPENCV, st.SPHERICAL, st.FISHEYE624, st.EUCM)   # the composition the op documents for OPENCV / Fisheye624 members
CROSS_F = 56.0                                         # the source views' focal length: wider than the reference's 80, so that more of it is in all of them
VISIBLE_TOL = 1e-6


def cross_pose(i):
    T = np.eye(4)
    T[:3] = tr.pose(CROSS_EYES[i], CROSS_TARGET, CROSS_ROLLS[i]).astype(np.float64)
    U, _, Vt = np.linalg.svd(T[:3, :3])                          # the fp32 rotation made orthonormal in fp64, the camera centre kept
    c = -T[:3, :3].T @ T[:3, 3]
    T[:3, :3] = U @ Vt
    T[:3, 3] = -T[:3, :3] @ c
    return T


def cross_views(models, size=st.VIEW):
    """(the reference view: a Pinhole at the trajectory's middle pose, the four source views of `models` at the cross poses)"""
    H, W, f = size
    ref = st.view(st.PINHOLE, st.row(st.PINHOLE, H, W, f), H, W, st.POSE_MID)
    return ref, [st.view(m, st.row(m, H, W, CROSS_F), H, W, cross_pose(i)) for i, m in enumerate(models)]


def seen_from(world, hit, v, margin=1.0):
    """the oracle's verdict on world points [H,W,3] in view v -> dict(visible: inside the image by `margin` pixels, in front, nothing
    before it on the ray, and the pixel it lands on `smooth`; occluded: inside and in front with a surface more than 3 % before it;
    by_sphere: that surface is the sphere; u, v, depth: the projection and the model's depth, fp64)"""
    H, W = v["H"], v["W"]
    r = st.projective(v["model"], v["params"], v["P"], world.reshape(-1, 3), H, W)
    with np.errstate(all="ignore"):
        inside = r["front"] & (r["u"] >= margin) & (r["u"] <= W - margin) & (r["v"] >= margin) & (r["v"] <= H - margin)
        x, y = np.clip(np.floor(np.where(inside, r["u"], 0)).astype(int), 0, W - 1), np.clip(np.floor(np.where(inside, r["v"], 0)).astype(int), 0, H - 1)
        landing = v["smooth"][y, x]
        visible = inside & landing & (np.abs(r["sdf"]) < VISIBLE_TOL)
        occluded = inside & landing & (r["sdf"] < -0.03 * r["d"])
    sh = hit.shape
    return dict(visible=visible.reshape(sh) & hit, occluded=occluded.reshape(sh) & hit, by_sphere=(occluded & (r["ids"] == st.SPHERE)).reshape(sh) & hit,
                u=r["u"].reshape(sh), v=r["v"].reshape(sh), depth=r["d"].reshape(sh))


def cross_conditions(ref, srcs):
    """(the share of the reference's smooth pixels the sphere hides in some view, the share visible in all views)"""
    seen = [seen_from(ref["world"], ref["hit"], v) for v in srcs]
    m = ref["smooth"]
    return (float(np.any([s["by_sphere"] for s in seen], axis=0)[m].mean()), float(np.all([s["visible"] for s in seen], axis=0)[m].mean()))


def warp_figures(out, uv, proj_depth, ref, src):
    """warp_camera(src's depth, depth=ref's depth, ...) against the oracle over the reference's smooth pixels: uv (mean, maximum) in pixels
    and proj_depth (mean signed, mean absolute, maximum) in voxels where the point lies inside the source image; the fetched depth
    against the analytic depth of the same point in the source view where the oracle says it is visible there"""
    s = seen_from(ref["world"], ref["hit"], src, margin=0.0)
    with np.errstate(all="ignore"):
        inside = ref["smooth"] & np.isfinite(s["u"]) & (s["u"] >= 0) & (s["u"] <= src["W"]) & (s["v"] >= 0) & (s["v"] <= src["H"]) & (s["depth"] > 0)
    e_uv = np.hypot(np.asarray(uv[0], np.float64) - s["u"], np.asarray(uv[1], np.float64) - s["v"])[inside]
    e_d = (np.asarray(proj_depth, np.float64) - s["depth"])[inside] / st.VOXEL
    vis = ref["smooth"] & seen_from(ref["world"], ref["hit"], src)["visible"]
    e_f = (np.asarray(out, np.float64) - s["depth"])[vis] / st.VOXEL
    return dict(uv=(float(e_uv.mean()), float(e_uv.max())), proj_depth=st.stats(e_d), fetched=st.stats(e_f), n=int(inside.sum()), visible=int(vis.sum()))


def consistency_figures(fused, count, consistent, ref, srcs):
    """depth_consistency's outputs ([H,W], [H,W], [V,H,W]) against the oracle over the reference's smooth pixels: the share of (pixel,
    view) pairs the oracle calls visible that are not consistent, the share it calls occluded that are consistent, over the pixels
    visible in all views the share whose count is not V and (mean signed, mean absolute, maximum) of fused - the analytic depth, voxels"""
    seen = [seen_from(ref["world"], ref["hit"], v) for v in srcs]
    m = ref["smooth"]
    vis = np.stack([s["visible"] for s in seen]) & m
    occ = np.stack([s["occluded"] for s in seen]) & m
    c = np.asarray(consistent, bool)
    everywhere = vis.all(axis=0)
    e = (np.asarray(fused, np.float64) - ref["depth"])[everywhere] / st.VOXEL
    return dict(missed=float((~c)[vis].mean()), leaked=float(c[occ].mean()), count=float((np.asarray(count)[everywhere] != len(srcs)).mean()),
                fused=st.stats(e), visible_all=float(everywhere[m].mean()), occluded=int(occ.sum()))


# ---- c. fusion -----------------------------------------------------------------------------------------------------------------------

def fusion_scene(views, T=None, origin=st.ORIGIN):
    """tsdf_common's scene dict of views (scene_truth.view dicts) for the host program; T [V,3,4] replaces the views' own poses"""
    V = len(views)
    H, W = views[0]["H"], views[0]["W"]
    T = np.stack([v["P"][:3] for v in views]) if T is None else np.asarray(T)
    return dict(B=1, V=V, Hs=H, Ws=W, grid=st.GRID, voxel=tc.f32(st.VOXEL), trunc=tc.f32(st.TRUNC), origin=np.array(origin, F)[None],
                depths=np.stack([v["depth"] for v in views]).astype(F)[None], models=tuple((v["model"],) for v in views),
                params=np.stack([v["params"][None] for v in views]).astype(F), T=T.astype(F))


def projective_truth(views):
    """per voxel of the grid, from the TRUE views: truth (the mean over the observing views of min(sdf, trunc), in the volume's units),
    n_obs, and clear: no view's decision hangs on the discretisation -- the projection further than a pixel from the image's border,
    sdf further than a voxel from -trunc, and the nearest pixel `smooth` (no crease or silhouette within SMOOTH_K pixels)"""
    p = st.voxel_centres()
    acc, n_obs, clear = np.zeros(len(p)), np.zeros(len(p), int), np.ones(len(p), bool)
    for v in views:
        H, W = v["H"], v["W"]
        r = st.projective(v["model"], v["params"], v["P"], p, H, W)
        with np.errstate(all="ignore"):
            inside = r["front"] & (r["u"] >= 0) & (r["u"] < W) & (r["v"] >= 0) & (r["v"] < H)
            border = r["front"] & ((np.abs(r["u"]) < 1) | (np.abs(r["u"] - W) < 1) | (np.abs(r["v"]) < 1) | (np.abs(r["v"] - H) < 1))
            x = np.clip(np.floor(np.where(inside, r["u"], 0)).astype(int), 0, W - 1)
            y = np.clip(np.floor(np.where(inside, r["v"], 0)).astype(int), 0, H - 1)
            obs = inside & (r["sdf"] >= -st.TRUNC)
            clear &= ~border & ~(inside & ~v["smooth"][y, x]) & ~(inside & (np.abs(r["sdf"] + st.TRUNC) < st.VOXEL))
            acc += np.where(obs, np.minimum(r["sdf"], st.TRUNC), 0.0)
        n_obs += obs
    return dict(truth=acc / np.maximum(n_obs, 1), n_obs=n_obs, clear=clear, centres=p)


def fusion_figures(tsdf, weight, truth):
    """tsdf, weight [Nz,Ny,Nx] against projective_truth(): (mean signed, mean absolute, maximum) of tsdf * trunc - truth in voxels over
    the voxels with weight > 0, |tsdf| < 0.5 and a clear truth; the share of those voxels among all with weight > 0 and |tsdf| < 0.5;
    the share of voxels further than a voxel from the surface (Euclidean) whose sign is not sdf(centre)'s; the share whose weight is
    not the number of observing views"""
    t, w = np.asarray(tsdf, np.float64).reshape(-1), np.asarray(weight, np.float64).reshape(-1)
    band = (w > 0) & (np.abs(t) < 0.5)
    cmp_ = band & truth["clear"] & (truth["n_obs"] > 0)
    e = (t * st.TRUNC - truth["truth"])[cmp_] / st.VOXEL
    d = st.sdf(truth["centres"])
    far = (w > 0) & truth["clear"] & (np.abs(d) > st.VOXEL)
    wrong = far & ((t < 0) != (d < 0))
    counted = truth["clear"] & (truth["n_obs"] > 0)
    return dict(err=st.stats(e) if cmp_.any() else (np.nan,) * 3, compared=float(cmp_.sum() / max(band.sum(), 1)), n=int(cmp_.sum()),
                sign=float(wrong.sum() / max(far.sum(), 1)), weight=float((w != truth["n_obs"])[counted].mean()))


# ---- d. surface ----------------------------------------------------------------------------------------------------------------------

def surface_figures(vertices, normals=None, faces=None):
    """world points [N,3] (a mesh's vertices or tsdf_points' cloud) against the scene: (mean signed, mean absolute, maximum) of
    sdf(vertex) in voxels and, with normals, (mean, maximum) of the angle to normal(vertex) in degrees, over the vertices further than
    CREASE_K voxels from a crease; the share compared; each element's share of the compared; with faces the share of triangles (centroid
    outside the crease band) whose face normal does not agree with the analytic normal at the centroid"""
    p = np.asarray(vertices, np.float64)
    keep = st.crease_distance(p) > CREASE_K * st.VOXEL
    out = dict(err=st.stats(st.sdf(p[keep]) / st.VOXEL), compared=float(keep.mean()), shares=st.element_shares(st.element(p[keep])), n=len(p))
    if normals is not None:
        a = st.angle_deg(np.asarray(normals, np.float64)[keep], st.normal(p[keep]), axis=1)
        out["angle"] = (float(a.mean()), float(a.max()))
    if faces is not None:
        tri = p[np.asarray(faces, np.int64)]
        c = tri.mean(axis=1)
        fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        ok = st.crease_distance(c) > CREASE_K * st.VOXEL
        out["wound_wrong"] = float(((fn * st.normal(c)).sum(1) <= 0)[ok].mean())
        out["triangles"] = int(ok.sum())
    return out


# ---- e. rendering --------------------------------------------------------------------------------------------------------------------

def observed(world, hit, views):
    """pixels whose analytic hit lies inside the grid by two voxels and is seen by some fused view: it projects into that view's image,
    a pixel from its border, onto a `smooth` pixel, and nothing lies in front of it"""
    lo = np.array(st.ORIGIN) + 2 * st.VOXEL
    hi = np.array(st.ORIGIN) + (np.array(st.GRID[::-1]) - 2) * st.VOXEL
    inside = hit & ((world >= lo) & (world <= hi)).all(axis=-1)
    seen = np.zeros(hit.shape, bool)
    p = world.reshape(-1, 3)
    for v in views:
        H, W = v["H"], v["W"]
        r = st.projective(v["model"], v["params"], v["P"], p, H, W)
        with np.errstate(all="ignore"):
            ok = r["front"] & (r["u"] >= 1) & (r["u"] < W - 1) & (r["v"] >= 1) & (r["v"] < H - 1) & (np.abs(r["sdf"]) < 1e-6)
            x, y = np.clip(np.floor(np.where(ok, r["u"], 0)).astype(int), 0, W - 1), np.clip(np.floor(np.where(ok, r["v"], 0)).astype(int), 0, H - 1)
        seen |= (ok & v["smooth"][y, x]).reshape(hit.shape)
    return inside & seen


def render_figures(depth, valid, points, normals, truth, views):
    """a rendered view [H,W], [3,H,W] against scene_truth.view's `truth` of the same camera and pose, over the pixels valid in both and
    smooth: depth (mean signed, mean absolute, maximum) in voxels, points (mean, maximum distance) in voxels, normals (mean, maximum
    angle) in degrees; each element's share of the compared pixels; the share of invalid pixels among the smooth ones whose analytic
    hit lies in the observed part of the grid (`views`: the fused ones)"""
    valid = np.asarray(valid, bool)
    cmp_ = valid & truth["hit"] & truth["smooth"]
    obs = observed(truth["world"], truth["hit"], views) & truth["smooth"]
    e = (np.asarray(depth, np.float64) - truth["depth"])[cmp_] / st.VOXEL
    pe = np.linalg.norm(np.asarray(points, np.float64) - truth["points"], axis=0)[cmp_] / st.VOXEL
    has_n = cmp_ & (np.asarray(normals) != 0).any(axis=0)
    a = st.angle_deg(np.asarray(normals, np.float64)[:, has_n], truth["normals"][:, has_n])
    return dict(depth=st.stats(e), points=(float(pe.mean()), float(pe.max())), angle=(float(a.mean()), float(a.max())),
                shares=st.element_shares(truth["ids"][cmp_]), invalid=float((~valid)[obs].mean()), observed=int(obs.sum()), n=int(cmp_.sum()),
                no_normal=float(1 - has_n.sum() / max(cmp_.sum(), 1)))


def render_truths(size=st.VIEW):
    """(model, pose index, the oracle's view) of section e: the four closed-form models, alternating between the two poses of RENDERED"""
    H, W, f = size
    return [(m, st.RENDERED[i % 2], st.view(m, st.row(m, H, W, f), H, W, st.trajectory()[st.RENDERED[i % 2]])) for i, m in enumerate(st.CLOSED)]


# ---- f. the loop ---------------------------------------------------------------------------------------------------------------------

LOOP = dict(iters=8, dist_tol=0.2)


def frame_view(model, k, size=st.FRAME):
    H, W, f = size
    return st.view(model, st.row(model, H, W, f), H, W, st.trajectory()[k])


def compose_track(E, prior):
    """TsdfVolume.track's result in numpy fp32: invert_rigid(E) . prior, element-wise as its docstring spells it"""
    A, Bm = tr.invert(np.asarray(E, F)), np.asarray(prior, F)[:3]
    out = np.zeros((3, 4), F)
    for i in range(3):
        out[i] = (A[i, 0] * Bm[0] + A[i, 1] * Bm[1]) + A[i, 2] * Bm[2]
        out[i, 3] = out[i, 3] + A[i, 3]
    return out


# ---- the chain through the host programs -----------------------------------------------------------------------------------------------

def host_volume(exe, views, T=None, origin=st.ORIGIN, volume=None):
    """tests/tsdf_host on views -> tsdf_render_common's volume dict"""
    s = fusion_scene(views, T, origin)
    r = tc.host_tsdf(exe, s, volume=None if volume is None else (volume["tsdf"], volume["weight"], None))
    return dict(tsdf=r["tsdf"], weight=r["weight"], color=None, origin=np.array(s["origin"], F), voxel=s["voxel"], grid=s["grid"], B=1,
                count=r["count"], live=r["live"], xyz=r["xyz"])


def host_mesh(exe, vol):
    r = tm.host_cells(exe, vol["tsdf"], vol["weight"], None, vol["origin"], vol["voxel"], 1.0)
    return tm.packed(r)


def host_render_view(exe, vol, truth, P=None):
    """tests/tsdf_render_host from the truth's camera at the world-to-camera pose P (the truth's own without one)"""
    P = truth["P"] if P is None else P
    T_cv = tr.invert(np.asarray(P, F)[None, :3])
    r = tr.host_render(exe, vol, [truth["model"]], truth["params"][None], (truth["H"], truth["W"]), T_cv=T_cv, near=st.NEAR, far=st.FAR, colour=False)
    return dict(depth=r["depth"][0, 0], valid=r["valid"][0, 0], points=r["points"][0], normals=r["normals"][0])


def host_loop(exes, model, n_frames, compose=compose_track, negate_normals=False, cos_tol=None):
    """the advertised loop through the host programs: frame 0 integrated at its true pose, then per frame the volume rendered at the prior
    pose, icp_host's LOOP["iters"] steps from the identity against that prediction, the pose composed and the frame integrated with it.
    exes = (tsdf_host, tsdf_render_host, icp_host) -> (poses [n_frames,3,4] fp32, per frame (status all 1, the matched share of the
    last step), the final volume)"""
    e_tsdf, e_render, e_icp = exes
    T = st.trajectory()
    frames = [frame_view(model, k) for k in range(n_frames + 1)]
    vol = host_volume(e_tsdf, [frames[0]])
    poses, info = [np.asarray(T[0][:3], F)], []
    for k in range(1, n_frames + 1):
        fr = frames[k]
        pred = host_render_view(e_render, vol, fr, P=poses[-1])
        depth = fr["depth"].astype(F)
        kw = {}
        if cos_tol is not None:
            n = fr["normals"].astype(F)
            kw = dict(cos_tol=cos_tol, normals=(-n if negate_normals else n)[None])
        r = ic.host_run(e_icp, depth=depth[None], params=fr["params"][None], models_frame=[model], mp=pred["points"][None], mn=pred["normals"][None],
                        mv=pred["valid"].astype(np.uint8)[None], params_model=fr["params"][None], models_model=[model], T=np.eye(4, dtype=F)[None, :3],
                        dist_tol=LOOP["dist_tol"], iters=LOOP["iters"], **kw)
        S = r["systems"][-1, 0]
        poses.append(compose(r["Ts"][-1, 0], poses[-1]))
        info.append((bool((r["status"] == 1).all()), float(S[29] / max((depth > 0).sum(), 1))))
        vol = host_volume(e_tsdf, [fr], T=poses[-1][None], volume=vol)
    return np.stack(poses), info, vol


def pose_figures(poses, start=0):
    """per frame (rotation error in degrees, translation error) against the trajectory"""
    T = st.trajectory()
    return [ic.pose_errors(p, T[start + k]) for k, p in enumerate(poses)]
