"""The analytic scene the reconstruction chain is measured against (not a test module): a room corner of three planes with a sphere in
front of it, seen through any of the six camera models from any pose, in fp64 numpy.  Nothing here is a discretisation and nothing is
shared with the kernels or their restatements: the surfaces are intersected in closed form.  The only camera arithmetic is the fp64
restatement the repository already pins against the reference -- tools/make_golden_gt_points.py: restate for the rays and
tools/make_golden_camera_project.py: project_model for the way back -- so no camera formula is written a second time.

    sdf(p), normal(p), element(p)      the signed distance (positive in free space), the normal and the id of the nearest surface element
    rays(model, params, H, W)          the unit directions of the pixel centres
    view(model, params, H, W, P)       depth, points, normals, hit, id and `smooth` of the scene seen from the world-to-camera pose P
    projective(model, params, P, p)    what tsdf_integrate's definition implies for world points p in one view: the model's depth of the
                                       surface along the ray through p minus the model's depth of p
    TRAJECTORY                         13 world-to-camera poses, 1.5 degrees and 0.038 apart
    planted defects                    view(..., centre_shift=) and spherical_as_z() corrupt a view the way a kernel bug would"""
import functools

import numpy as np

import camera_project_common as cpc
import gt_points_common as gpc
import icp_common as ic
import tsdf_common as tc

gp, cp = gpc.gp, cpc.cp
PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = ic.MODELS
MODELS, CLOSED, NAMES = ic.MODELS, ic.CLOSED, ic.NAMES

# ---- the scene ---------------------------------------------------------------------------------------------------------------------

PLANES = ic.PLANES                                     # x = -1.2, y = 1.0, z = 3.0: the free space is x > -1.2, y < 1.0, z < 3.0
PLANE_SIGN = (1.0, -1.0, -1.0)                         # the normal of each plane along its axis, pointing into the free space
SPHERE_C, SPHERE_R = np.array([0.2, 0.3, 2.0]), 0.5    # 0.2 from the plane y = 1, 0.5 from z = 3
SPHERE = 3                                             # the element ids: 0, 1, 2 the planes in PLANES' order, 3 the sphere
ELEMENTS = ("x=-1.2", "y=1.0", "z=3.0", "sphere")
SMOOTH_K = 2

# the volume of tests/test_icp_gpu.py's end-to-end test: 40 x 40 x 48 voxels of 5/64, x in -1.5 .. 1.625, y in -1.9 .. 1.225, z in 0 .. 3.75
VOXEL = 0.078125
GRID = (48, 40, 40)                                    # (Nz, Ny, Nx)
ORIGIN = (-1.5, -1.9, 0.0)
TRUNC = 0.25                                           # 3.2 voxels
VIEW = (96, 128, 80.0)                                 # H, W and the focal length a pinhole of that view would have
FRAME = (48, 64, 40.0)                                 # the tracked frames and the rendered predictions
NEAR, FAR = 0.3, 5.0


def _distances(p):
    """the four element distances of points p [...,3] -> [4,...]"""
    p = np.asarray(p, np.float64)
    planes = [PLANE_SIGN[k] * (p[..., axis] - value) for k, (axis, value) in enumerate(PLANES)]
    return np.stack(planes + [np.linalg.norm(p - SPHERE_C, axis=-1) - SPHERE_R])


def sdf(p):
    """the signed distance of world points [...,3] to the scene: exact wherever it is >= 0 (the solid is a union), negative inside"""
    return _distances(p).min(axis=0)


def element(p):
    return np.abs(_distances(p)).argmin(axis=0)


def crease_distance(p):
    """how far the second nearest element is: small next to a crease or where the sphere comes close to a plane"""
    return np.sort(np.abs(_distances(p)), axis=0)[1]


def normal(p, ids=None):
    """the analytic normal of the nearest element (or of element ids) at world points [...,3], pointing into the free space"""
    p = np.asarray(p, np.float64)
    ids = element(p) if ids is None else ids
    n = np.zeros(p.shape)
    for k, (axis, _) in enumerate(PLANES):
        n[..., axis] = np.where(ids == k, PLANE_SIGN[k], n[..., axis])
    r = p - SPHERE_C
    r = r / np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), 1e-300)
    return np.where((ids == SPHERE)[..., None], r, n)


def cast(c, w):
    """rays from c [3] along unit directions w [...,3] -> (s [...] the distance to the nearest surface, inf without one, ids [...], -1)"""
    w = np.asarray(w, np.float64)
    best, ids = np.full(w.shape[:-1], np.inf), np.full(w.shape[:-1], -1)
    with np.errstate(all="ignore"):
        for k, (axis, value) in enumerate(PLANES):
            s = (value - c[axis]) / w[..., axis]
            hit = (s > 0) & (s < best)
            best, ids = np.where(hit, s, best), np.where(hit, k, ids)
        oc = c - SPHERE_C
        b = (w * oc).sum(-1)
        disc = b * b - (oc @ oc - SPHERE_R ** 2)
        s = -b - np.sqrt(disc)                                             # the near root; the camera is never inside the sphere
        hit = (disc > 0) & (s > 0) & (s < best)
        best, ids = np.where(hit, s, best), np.where(hit, SPHERE, ids)
    return best, ids


# ---- the cameras -------------------------------------------------------------------------------------------------------------------

def row(model, H, W, f):
    return tc.row_for(model, H, W, f)


def rays(model, params, H, W):
    """unit directions of the pixel centres fp64 [3,H,W]: the pinned fp64 restatement of reconstruct at depth 1, normalised"""
    p = gp.restate(np.ones((1, H, W), np.float32), np.asarray(params, np.float32)[None], [model], np.float64)[0]
    return p / np.linalg.norm(p, axis=0)


def model_depth(model, q):
    """the model's depth of camera-frame points [3,...]: the distance for Spherical, z otherwise"""
    return np.linalg.norm(q, axis=0) if model == SPHERICAL else q[2]


def project(model, params, q):
    """camera-frame points [3,...] -> (u, v) through the pinned fp64 restatement of project"""
    p = np.asarray(params, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return cp.project_model(model, p, q[0], q[1], q[2], np.float64)


def shifted(params, du, dv):
    """the row with the principal point moved: a view GENERATED with it looks like one whose pixels sit (du, dv) off their centres.
    Spherical has no principal point and is returned as it is."""
    out = np.array(params, np.float32)
    out[2] += du
    out[3] += dv
    return out


def _same_in_window(ids, k):
    """pixels whose whole (2k+1)^2 neighbourhood inside the image carries their own id"""
    H, W = ids.shape
    ok = np.ones((H, W), bool)
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            ok[yd, xd] &= ids[ys, xs] == ids[yd, xd]
    return ok


def view(model, params, H, W, P, k=SMOOTH_K, centre_shift=None):
    """the scene seen through (model, params) from the world-to-camera pose P [4,4] or [3,4] -> dict, all fp64:
    depth [H,W] the model's depth (0 without a hit), points [3,H,W] and normals [3,H,W] in the camera frame, hit bool, ids (-1 without a
    hit), smooth bool: hit and no other id (crease, silhouette, no hit) within k pixels, from the ids alone; s the distance along the ray.
    centre_shift = (du, dv) plants a defect: the view is generated with the principal point moved, the caller keeps the true row."""
    P = np.asarray(P, np.float64)
    R, t = P[:3, :3], P[:3, 3]
    d = rays(model, params if centre_shift is None else shifted(params, *centre_shift), H, W)
    s, ids = cast(-R.T @ t, np.einsum("ji,jhw->hwi", R, d))
    hit = np.isfinite(s)
    pts = np.where(hit, d * np.where(hit, s, 0.0), 0.0)
    world = np.einsum("ji,jhw->hwi", R, pts - t[:, None, None])
    nrm = np.where(hit, np.einsum("ij,hwj->ihw", R, normal(world, ids)), 0.0)
    return dict(depth=np.where(hit, model_depth(model, pts), 0.0), points=pts, normals=nrm, hit=hit, ids=ids, s=s,
                smooth=hit & _same_in_window(ids, k), world=world, model=model, params=np.asarray(params, np.float32), P=P, H=H, W=W)


def spherical_as_z(v):
    """defect 4: a Spherical view's depth written as z"""
    assert v["model"] == SPHERICAL
    return np.where(v["hit"], v["points"][2], 0.0)


def projective(model, params, P, p, H, W):
    """tsdf_integrate's definition for world points p [N,3] in one view, with the analytic surface in place of the depth map's nearest
    pixel: q = P p, the ray from the camera through q cast into the scene, sdf = depth(surface) - depth(q) in the model's depth.
    -> dict(sdf [N], ids [N], u, v [N] the projection, d [N] the point's depth, front: d > 0 and a surface on the ray)"""
    P = np.asarray(P, np.float64)
    R, t = P[:3, :3], P[:3, 3]
    q = (np.asarray(p, np.float64) @ R.T + t).T
    n = np.linalg.norm(q, axis=0)
    w = q / n
    s, ids = cast(-R.T @ t, (w.T @ R))
    d = model_depth(model, q)
    with np.errstate(all="ignore"):
        ds = model_depth(model, w * s)
        u, v = project(model, params, q)
    return dict(sdf=ds - d, ids=ids, u=u, v=v, d=d, front=(d > 0) & np.isfinite(s) & (q[2] > 0))


def voxel_centres(grid=GRID, voxel=VOXEL, origin=ORIGIN):
    """[Nz*Ny*Nx,3], x fastest: origin + (index + 0.5) * voxel"""
    Nz, Ny, Nx = grid
    z, y, x = np.meshgrid(*(((np.arange(n) + 0.5) * voxel) for n in (Nz, Ny, Nx)), indexing="ij")
    return np.stack([x + origin[0], y + origin[1], z + origin[2]], axis=-1).reshape(-1, 3)


# ---- the poses ---------------------------------------------------------------------------------------------------------------------

STEP = ic.pose((0.012, -0.020, 0.012), (0.027, -0.016, 0.0215))            # 1.50 degrees, 0.0380: half of what track_camera is shown to recover
N_FRAMES = 13
POSE_MID = ic.pose((0.06, -0.12, 0.03), (0.05, 0.1, 0.15))


@functools.lru_cache(maxsize=None)
def trajectory():
    """N_FRAMES world-to-camera poses T_k = STEP^(k - 6) POSE_MID: rotations about all three axes, translations along none of them"""
    T = [np.linalg.matrix_power(np.linalg.inv(STEP), 6) @ POSE_MID]
    for _ in range(N_FRAMES - 1):
        T.append(STEP @ T[-1])
    return tuple(T)


INTEGRATED = (0, 2, 4, 6, 8, 10)                       # the trajectory's poses the fused views are taken from, one per model in MODELS' order
RENDERED = (3, 9)                                      # and the poses the volume is rendered from: none of the above


def invert(T):
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
    return out


@functools.lru_cache(maxsize=None)
def fused_views(defect=None):
    """the six views of section c: model MODELS[i] at trajectory()[INTEGRATED[i]], VIEW's size.  defect: None, "half_pixel" (the
    principal point off by half a pixel in u), "corners" (pixel corners for centres: off by half a pixel in u and v), "as_z" (the
    Spherical view's depth written as z).  Spherical has no principal point; the first two leave it as it is."""
    H, W, f = VIEW
    shift = {None: None, "as_z": None, "half_pixel": (0.5, 0.0), "corners": (0.5, 0.5)}[defect]
    out = []
    for i, m in enumerate(MODELS):
        v = view(m, row(m, H, W, f), H, W, trajectory()[INTEGRATED[i]], centre_shift=None if m == SPHERICAL else shift)
        if defect == "as_z" and m == SPHERICAL:
            v = dict(v, depth=spherical_as_z(v))
        out.append(v)
    return tuple(out)


# ---- figures -----------------------------------------------------------------------------------------------------------------------

def angle_deg(a, b, axis=0):
    """the angle between unit vectors along `axis`, through atan2 so that small angles resolve"""
    c = (a * b).sum(axis)
    s = np.linalg.norm(np.cross(a, b, axis=axis), axis=axis)
    return np.degrees(np.arctan2(s, c))


def stats(e):
    """(mean signed, mean absolute, maximum absolute) of an error array"""
    e = np.asarray(e, np.float64).reshape(-1)
    return float(e.mean()), float(np.abs(e).mean()), float(np.abs(e).max())


def element_shares(ids):
    ids = np.asarray(ids).reshape(-1)
    return [float((ids == k).mean()) for k in range(4)]
