"""What the depth_consistency tests share (not a test module): geometrically consistent scenes -- a tilted plane seen by a reference view
and V neighbour views through any of the four closed-form camera models, with a third of every view's pixels pushed off the plane, holes
and special values -- the call of the host program tests/consistency_host/consistency_host.cpp, the known-answer scene, and the helpers of
the GPU tests.  The oracle of the GPU tests is unidepth_amd.consistency.depth_consistency_composition, the merged calls in a loop, never
the fused kernel."""
import functools

import numpy as np

import host_program
from host_program import ROOT, bits, f32_bits  # noqa: F401  (the tests reach them through this module)

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = 1, 2, 3, 4, 5, 6
NAMES = {PINHOLE: "pinhole", EUCM: "eucm", SPHERICAL: "spherical", MEI: "mei"}
CLOSED = (PINHOLE, EUCM, SPHERICAL, MEI)
PX_TOL, REL_TOL = 1.0, 0.01
PLANE_N, PLANE_C = np.array([-0.12, 0.08, 1.0]), 5.0          # n . X = c in the reference camera's frame: z = 5 + 0.12 x - 0.08 y


def rows_for(model, H, W, hfov):
    """one 16-float parameter row of `model` for an H x W image seeing about +-hfov radians horizontally"""
    f = (W / 2) / np.tan(hfov)
    cx, cy = W / 2 + 0.1, H / 2 - 0.2
    row = np.zeros(16, np.float32)
    if model == PINHOLE:
        row[:4] = [f, 1.02 * f, cx, cy]
    elif model == EUCM:
        row[:6] = [f, 1.02 * f, cx, cy, 0.5, 1.0]
    elif model == SPHERICAL:
        row[:8] = [f, f, cx, cy, max(W, 2), max(H, 2), hfov, np.arctan(np.tan(hfov) * H / W)]      # the model divides by W - 1 and H - 1
    elif model == MEI:
        row[:9] = [1.9 * f, 1.93 * f, cx, cy, -0.05, 0.01, 1e-3, -1e-3, 0.9]
    else:
        raise ValueError(model)
    return row


def depth_one_points(model, p, H, W):
    """float64 [H,W,3]: the point each pixel centre reconstructs to with a depth of 1 (the model's depth: z, the distance for Spherical).
    A float64 restatement that is only as good as a scene needs (the tests' tolerances are 1 pixel and 1 %), not an oracle."""
    p = p.astype(np.float64)
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    if model == SPHERICAL:
        lon = (u - (p[4] - 1) / 2) / (p[4] - 1) * (2 * p[6])
        lat = (v - (p[5] - 1) / 2) / (p[5] - 1) * (2 * p[7])
        return np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], axis=-1)
    mx, my = (u - p[2]) / p[0], (v - p[3]) / p[1]
    if model == PINHOLE:
        mz = np.ones_like(mx)
    elif model == EUCM:
        al, be = p[4], p[5]
        r2 = mx * mx + my * my
        mz = (1 - be * al * al * r2) / (al * np.sqrt(np.maximum(1 - (2 * al - 1) * be * r2, 1e-5)) + (1 - al))
    else:                                                       # MEI: undo the distortion by fixed-point iteration, lift with xi
        k1, k2, p1, p2, xi = p[4:9]
        x, y = mx.copy(), my.copy()
        for _ in range(30):
            r2 = x * x + y * y
            rad = 1 + k1 * r2 + k2 * r2 * r2
            tx = (2 * x * x + r2) * p1 + 2 * x * y * p2
            ty = (2 * y * y + r2) * p2 + 2 * x * y * p1
            x, y = (mx - tx) / rad, (my - ty) / rad
        rho2 = x * x + y * y
        mz = 1 - xi * (rho2 + 1) / (xi + np.sqrt(1 + (1 - xi * xi) * rho2))
        mx, my = x, y
    return np.stack([mx / mz, my / mz, np.ones_like(mx)], axis=-1)


def _pose(g):
    """a small rigid motion [3,4]: a rotation of at most 0.04 rad about a random axis and a translation of at most 0.25 per axis"""
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = g.uniform(-0.04, 0.04)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    return np.concatenate([R, g.uniform(-0.25, 0.25, size=(3, 1))], axis=1).astype(np.float32)


def view_models(ref_models, V):
    """models[v][b]: image b of view v; every image meets V different models, every model appears in every view of a batch of four"""
    return tuple(tuple(CLOSED[(b + v + 1) % 4] for b in range(len(ref_models))) for v in range(V))


@functools.lru_cache(maxsize=None)
def scene(ref_models, V=3, H=13, W=17, Hs=11, Ws=19, per_image=False, src_models=None, seed=0):
    """The tilted plane seen by a reference batch of the models `ref_models` and V views (view_models unless src_models[v][b] is given),
    numpy, read-only.  depth [B,1,H,W] with 6 % holes (0, negative, NaN), valid_in [B,H,W] (6 % zeros), src_depths [B,V,Hs,Ws] -- the
    plane's depth in each view, with every third 4x4 block pushed 10 % off the plane and 4 % holes (0, NaN, negative) -- src_masks
    [B,V,Hs,Ws] (8 % zeros), the parameter rows, and transforms [V,3,4] (shared) or [B,V,3,4]."""
    B = len(ref_models)
    g = np.random.RandomState(9400 + seed)
    models_src = src_models if src_models is not None else view_models(ref_models, V)
    params_ref = np.stack([rows_for(m, H, W, 0.45) for m in ref_models])
    params_src = np.stack([np.stack([rows_for(models_src[v][b], Hs, Ws, 0.40) for b in range(B)]) for v in range(V)])
    T = np.stack([_pose(g) for _ in range(V)])
    T = np.stack([np.stack([_pose(g) for _ in range(V)]) for _ in range(B)]) if per_image else T
    depth = np.empty((B, 1, H, W), np.float32)
    src = np.empty((B, V, Hs, Ws), np.float32)
    ys, xs = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    off_plane = ((ys // 4 + xs // 4) % 3) == 0
    for b in range(B):
        depth[b, 0] = PLANE_C / (depth_one_points(ref_models[b], params_ref[b], H, W) @ PLANE_N)
        for v in range(V):
            t = (T[b, v] if per_image else T[v]).astype(np.float64)
            n2 = t[:, :3] @ PLANE_N                                            # the plane in the view's frame: n2 . X = c + n2 . t
            s = (PLANE_C + n2 @ t[:, 3]) / (depth_one_points(models_src[v][b], params_src[v, b], Hs, Ws) @ n2)
            src[b, v] = np.where(off_plane, 1.1 * s, s)
    hole = g.uniform(size=depth.shape)
    depth[hole < 0.02] = 0.0
    depth[(hole >= 0.02) & (hole < 0.04)] = -1.5
    depth[(hole >= 0.04) & (hole < 0.06)] = np.nan
    h = g.uniform(size=src.shape)
    src[h < 0.02] = 0.0
    src[(h >= 0.02) & (h < 0.03)] = np.nan
    src[(h >= 0.03) & (h < 0.04)] = -2.0
    d = dict(B=B, V=V, H=H, W=W, Hs=Hs, Ws=Ws, depth=depth, valid_in=(g.uniform(size=(B, H, W)) >= 0.06).astype(np.uint8), src_depths=src,
             src_masks=(g.uniform(size=src.shape) >= 0.08).astype(np.uint8), models_ref=tuple(ref_models), models_src=models_src,
             params_ref=params_ref, params_src=params_src, T=T)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


MIXED = (MEI, SPHERICAL, EUCM, PINHOLE)
BIG = dict(H=37, W=53, Hs=29, Ws=41)                           # 1961 reference pixels: seven full workgroups and a partial one
# name -> (scene arguments, call arguments): reference pixel counts around the wave's and the workgroup's edges as 1 x n images, tiny
# sources, one view, and B * V = 256 with 2x2 images.  A source of a few pixels holds one depth for a whole region of the plane, so those
# scenes are judged at a rel_tol of 10 % (the plane's depth varies by about +-8 % over the image).
EDGES = {f"n{n}": (dict(ref_models=MIXED, H=1, W=n, per_image=True), {}) for n in (1, 63, 64, 65, 255, 256, 257)}
EDGES.update({"src1x1": (dict(ref_models=MIXED, Hs=1, Ws=1), dict(rel_tol=0.1)), "src2x3": (dict(ref_models=MIXED, Hs=2, Ws=3), dict(rel_tol=0.1)),
              "v1": (dict(ref_models=MIXED, V=1), {}),
              "limit": (dict(ref_models=CLOSED * 16, V=4, H=2, W=2, Hs=2, Ws=3), dict(rel_tol=0.1))})


def assert_edge_shares(name, consistent):
    """assert_shares for an EDGES scene; the single reference pixel of "n1" has no share of its own: some of its B * V decisions are true
    and some are false"""
    if name == "n1":
        assert consistent.any() and not consistent.all()
    else:
        assert_shares(consistent, name)


def invert(T):
    """unidepth_amd.consistency.invert_rigid on a numpy array (plain torch, runs on the CPU)"""
    import torch
    from unidepth_amd import consistency
    return consistency.invert_rigid(torch.from_numpy(np.array(T, np.float32, order="C"))).numpy()


def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "consistency_host")


def host_consistency(exe, depth, params_ref, models_ref, src_depths, params_src, models_src, T, *, px_tol=PX_TOL, rel_tol=REL_TOL, min_views=1,
                     valid_in=None, src_masks=None):
    """tests/consistency_host: the fused per-pixel function on numpy inputs, after the program has checked it against the chain of the
    separate functions (exit status 3 when they differ, a sanitizer report otherwise).  T is [V,3,4] or [B,V,3,4].
    -> dict(fused [B,H,W], count [B,H,W] uint8, mask bool [B,H,W], consistent bool [B,V,H,W], err_px, err_rel [B,V,H,W])"""
    B, (H, W) = depth.shape[0], depth.shape[-2:]
    _, V, Hs, Ws = src_depths.shape
    Tn = np.ascontiguousarray(T, np.float32).reshape(-1, V, 3, 4)
    blobs = [np.ascontiguousarray(depth, np.float32).tobytes(), np.ascontiguousarray(params_ref, np.float32).tobytes(),
             np.ascontiguousarray(src_depths, np.float32).tobytes()]
    blobs += [np.ascontiguousarray(src_masks, np.uint8).tobytes()] if src_masks is not None else []
    blobs += [np.ascontiguousarray(params_src, np.float32).tobytes(), Tn.tobytes(), np.ascontiguousarray(invert(Tn)).tobytes()]
    blobs += [np.ascontiguousarray(valid_in, np.uint8).tobytes()] if valid_in is not None else []
    args = [B, V, H, W, Hs, Ws, Tn.shape[0], int(valid_in is not None), int(src_masks is not None), min_views, f32_bits(px_tol), f32_bits(rel_tol)]
    args += list(models_ref) + [models_src[v][b] for v in range(V) for b in range(B)]
    n = B * H * W
    parts = host_program.run(exe, args, blobs, [4 * n, n, n, V * n, 4 * V * n, 4 * V * n])
    return dict(fused=np.frombuffer(parts[0], np.float32).reshape(B, H, W), count=np.frombuffer(parts[1], np.uint8).reshape(B, H, W),
                mask=np.frombuffer(parts[2], np.uint8).reshape(B, H, W).astype(bool),
                consistent=np.frombuffer(parts[3], np.uint8).reshape(B, V, H, W).astype(bool),
                err_px=np.frombuffer(parts[4], np.float32).reshape(B, V, H, W), err_rel=np.frombuffer(parts[5], np.float32).reshape(B, V, H, W))


def host_scene(exe, s, **kw):
    return host_consistency(exe, s["depth"], s["params_ref"], s["models_ref"], s["src_depths"], s["params_src"], s["models_src"], s["T"], **kw)


def assert_shares(consistent, what):
    """no case may pass vacuously: every view's consistent share, over the batch, lies strictly between 10 % and 90 %"""
    share = np.asarray(consistent, np.float64).mean(axis=(0, 2, 3))
    assert share.min() > 0.1 and share.max() < 0.9, (what, share.tolist())


# ---- the known answer ----------------------------------------------------------------------------------------------------------------

KA_SHIFTS = (4, -4, 8)                                        # the disparity of each view in pixels: fx * tx / z = 64 * (.25, -.25, .5) / 4
KA_BLOCK = (slice(2, 5), slice(12, 18))                       # the planted reference pixels, depth 4 * 1.1


def known_answer_inputs():
    """A fronto-parallel plane at z = 4, Pinhole cameras with fx = fy = 64 on both sides, views translated by +0.25, -0.25 and 0.5 along
    x: every intermediate is exact in fp32."""
    H, W, B, V = 8, 32, 2, 3
    row = np.zeros((B, 16), np.float32)
    row[:, :4] = [64.0, 64.0, 16.0, 4.0]
    T = np.zeros((V, 3, 4), np.float32)
    T[:, :, :3] = np.eye(3)
    T[:, 0, 3] = [0.25, -0.25, 0.5]
    depth = np.full((B, 1, H, W), 4.0, np.float32)
    planted = depth.copy()
    planted[(slice(None), 0) + KA_BLOCK] = np.float32(4.0) * np.float32(1.1)
    return dict(H=H, W=W, B=B, V=V, rows=row, rows_src=np.stack([row] * V), T=T, depth=depth, planted=planted,
                src_depths=np.full((B, V, H, W), 4.0, np.float32), models=(PINHOLE,) * B, models_src=((PINHOLE,) * B,) * V)


def check_known_answer(run):
    """run(depth, rel_tol) -> dict of numpy arrays as host_consistency returns them"""
    k = known_answer_inputs()
    W, V = k["W"], k["V"]
    x = np.arange(W)
    want = np.stack([(x + s >= 0) & (x + s <= W - 1) for s in KA_SHIFTS])               # [V,W]: the shifted pixel lies inside the source
    r = run(k["depth"], 0.01)
    assert np.array_equal(r["consistent"], np.broadcast_to(want[None, :, None, :], r["consistent"].shape))
    assert np.array_equal(r["count"], np.broadcast_to(want.sum(axis=0).astype(np.uint8), r["count"].shape))
    assert (r["count"] == V).any() and (r["count"] < V).any()
    assert (r["fused"] == 4.0).all() and r["mask"][r["count"] > 0].all() and not r["mask"][r["count"] == 0].any()
    assert not r["err_px"].any() and not r["err_rel"].any()
    blk = (slice(None),) + KA_BLOCK
    outside = np.ones(r["count"].shape, bool)
    outside[blk] = False
    r = run(k["planted"], 0.01)                                                          # |4 - 4.4| / 4.4 = 0.09 > 0.01
    assert not r["count"][blk].any() and not r["mask"][blk].any() and (r["fused"][blk] == k["planted"][0, 0][KA_BLOCK]).all()
    assert (r["fused"][outside] == 4.0).all() and not r["err_px"][:, :, outside[0]].any()
    e = r["err_rel"][(slice(None), slice(None)) + KA_BLOCK]
    assert (np.abs(e - 0.4 / 4.4) < 1e-6).all()
    r = run(k["planted"], 0.2)                                                           # 0.09 <= 0.2, and the point lands within a pixel
    assert (r["count"][blk] == V).all() and r["mask"][blk].all() and (r["err_px"][(slice(None), slice(None)) + KA_BLOCK] < 1.0).all()
    assert ((r["fused"][blk] > 4.0) & (r["fused"][blk] < 4.4)).all() and (r["fused"][outside] == 4.0).all()


# ---- special values ------------------------------------------------------------------------------------------------------------------

def special_case():
    """the per-image scene of a mixed reference batch with: NaN, +-inf, 0, -0.0, negative and 1e-30 at the head of the first two rows of
    every reference depth; NaN, +-inf, 0 and negative values spread over the views' depths; image 1's reference row a singular Pinhole
    (fx = 0); image 2's views singular Pinholes; image 3's transforms turned so that every point lies behind every view
    -> (scene dict with the changed arrays)"""
    s = dict(scene((MEI, PINHOLE, EUCM, SPHERICAL), per_image=True, seed=7))
    depth = np.array(s["depth"])
    depth[:, 0, 0, 0:4] = [0.0, -3.0, np.nan, np.inf]
    depth[:, 0, 1, 0:4] = [np.inf, -np.inf, -0.0, 1e-30]
    src = np.array(s["src_depths"])
    src[:, :, ::3, ::4] = np.nan
    src[:, :, 1::3, 1::4] = np.inf
    src[:, :, 2::3, 2::4] = -np.inf
    src[:, :, 2::3, 3::4] = 0.0
    params_ref, params_src, T = np.array(s["params_ref"]), np.array(s["params_src"]), np.array(s["T"])
    params_ref[1, 0] = 0.0
    models_src = tuple(tuple(PINHOLE if b == 2 else m for b, m in enumerate(row)) for row in s["models_src"])
    params_src[:, 2] = 0.0
    params_src[:, 2, 1:4] = [40.0, 9.0, 5.0]
    T[3, :, 2, :] = [0.0, 0.0, -1.0, 0.0]                                      # z' = -z for every pixel of image 3
    s.update(depth=depth, src_depths=src, params_ref=params_ref, params_src=params_src, T=T, models_src=models_src)
    return s


def check_special(r, s, min_views):
    """what must hold of any result on special_case(): no decision is true of a pixel whose inputs cannot support it"""
    d = s["depth"][:, 0]
    ref_ok = d > 0                                                             # false for NaN
    assert (r["fused"][~ref_ok] == 0).all() and not r["mask"][~ref_ok].any() and not r["count"][~ref_ok].any()
    assert not r["consistent"][np.broadcast_to(~ref_ok[:, None], r["consistent"].shape)].any()
    bad = ~np.isfinite(d)
    bad[1:4] = True                                                            # the singular reference, the singular views, the views behind
    assert not r["count"][bad].any() and not r["consistent"][np.broadcast_to(bad[:, None], r["consistent"].shape)].any()
    if min_views >= 1:
        assert not r["mask"][bad].any()
    agreed = r["count"] > 0                                                    # (a depth of +inf alone is its own "mean": ref_ok holds for it)
    assert np.isfinite(r["fused"][agreed]).all() and (r["fused"][agreed] > 0).all() and (r["fused"][r["mask"]] > 0).all()
    assert np.array_equal(r["count"], r["consistent"].sum(axis=1).astype(np.uint8))
    assert r["count"][0].any()                                                 # image 0 is an ordinary one


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------

def prepared(params, models):
    """a PreparedCamera on the GPU from numpy rows and model tags"""
    import torch
    from unidepth_amd import gtpoints
    return gtpoints.PreparedCamera(torch.from_numpy(np.array(params, np.float32, order="C")).cuda(), models)


OUTPUTS = ("fused", "count", "mask", "consistent", "err_px", "err_rel")


def assert_same(got, want, what="", names=OUTPUTS):
    host_program.assert_same(got, want, names, what)
