"""What the warp_camera tests share (not a test module): the seeded inputs of the 37x53 <- 29x41 cases, the call of the host program
tests/warp_host/warp_host.cpp, and the oracle of the GPU tests -- the composition of the already merged calls (unproject_camera,
project_camera, remap), never the fused kernel."""
import functools
import numpy as np

import host_program
from host_program import ROOT, bits, f32_bits as tol_bits  # noqa: F401  (the tests reach them through this module)

PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = 1, 2, 3, 4, 5, 6
NAMES = {PINHOLE: "pinhole", EUCM: "eucm", SPHERICAL: "spherical", OPENCV: "opencv", FISHEYE624: "fisheye624", MEI: "mei"}
CLOSED = (PINHOLE, EUCM, SPHERICAL, MEI)
MODES = {"nearest": 0, "bilinear": 1}
PADDINGS = {"zeros": 0, "border": 1}
HO, WO, HS, WS, B = 37, 53, 29, 41, 6                      # 1961 destination pixels: seven full workgroups and a partial one
TOL = 0.25

# One parameter row per model and view.  Destination rows see about +-27 x +-20 degrees, source rows about +-22 x +-16, so that without any
# motion a good part of the destination pixels falls outside the source image.
DST_ROWS = {
    PINHOLE: [50.0, 51.0, 26.0, 18.0],
    EUCM: [48.0, 49.0, 26.2, 18.8, 0.45, 1.05],
    SPHERICAL: [8.4, 11.8, 26.5, 18.5, 53.0, 37.0, 0.5, 0.36],
    OPENCV: [50.0, 51.0, 26.4, 18.3, -0.25, 0.08, -0.01, 0, 0, 0, 1e-3, -2e-3, 1e-3, 5e-4, -1e-3, 2e-4],
    FISHEYE624: [54.0, 54.5, 26.7, 18.2, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 0, 0, 0, 0, 0, 0],
    MEI: [100.0, 101.0, 26.3, 18.6, -0.1, 0.02, 1e-3, -1e-3, 0.9],
}
SRC_ROWS = {
    PINHOLE: [50.0, 51.0, 20.2, 14.1],
    EUCM: [49.0, 50.0, 20.4, 14.6, 0.55, 0.95],
    SPHERICAL: [6.5, 9.2, 20.5, 14.5, 41.0, 29.0, 0.40, 0.28],
    OPENCV: [50.0, 51.0, 20.5, 14.2, -0.22, 0.07, -0.008, 0, 0, 0, 1e-3, -2e-3, 1e-3, 5e-4, -1e-3, 2e-4],
    FISHEYE624: [53.0, 53.5, 20.7, 14.1, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 1e-3, -1e-3, 5e-4, 1e-4, -5e-4, 1e-4],
    MEI: [100.0, 101.0, 20.4, 14.5, -0.1, 0.02, 1e-3, -1e-3, 0.9],
}
SRC_MODELS = (PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI)          # the source batch holds all six
# name -> the destination models of the batch: each closed-form model against all six sources, one mixed batch, and (through the wrapper's
# points path) one with OPENCV / Fisheye624 members
DST_SETS = {
    "pinhole": (PINHOLE,) * B, "eucm": (EUCM,) * B, "spherical": (SPHERICAL,) * B, "mei": (MEI,) * B,
    "mixed": (MEI, SPHERICAL, EUCM, PINHOLE, EUCM, SPHERICAL),
    "iterative": (OPENCV, FISHEYE624, PINHOLE, FISHEYE624, OPENCV, MEI),
}
TRANSFORMS = ("none", "shared", "batch")
# (source dtype, C, output dtype, src_mask, normalize)
KINDS = {"f32_c1_mask_norm": (np.float32, 1, np.float32, True, True), "u8_c3": (np.uint8, 3, np.uint8, False, False),
         "u8_c3_f32": (np.uint8, 3, np.float32, False, False)}


def rows(models, table):
    out = np.zeros((len(models), 16), np.float32)
    for b, m in enumerate(models):
        out[b, :len(table[m])] = table[m]
    return out


def _pose(g):
    """a small rigid motion [3,4]: a rotation of at most 0.04 rad about a random axis and a translation of at most 0.25 per axis"""
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = g.uniform(-0.04, 0.04)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    return np.concatenate([R, g.uniform(-0.25, 0.25, size=(3, 1))], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, Ho=HO, Wo=WO, Hs=HS, Ws=WS):
    """the seeded inputs of a destination set, numpy, read-only: depth [B,1,Ho,Wo] (2 .. 10 with 6 % holes: 0, negative, NaN), valid_in
    [B,Ho,Wo] (6 % zeros), the parameter rows and model tags of both views, a shared and a per-image motion, and the source view's maps"""
    g = np.random.RandomState(9100 + sorted(DST_SETS).index(name))
    depth = g.uniform(2.0, 10.0, size=(B, 1, Ho, Wo)).astype(np.float32)
    hole = g.uniform(size=depth.shape)
    depth[hole < 0.02] = 0.0
    depth[(hole >= 0.02) & (hole < 0.04)] = -1.5
    depth[(hole >= 0.04) & (hole < 0.06)] = np.nan
    d = dict(depth=depth, valid_in=(g.uniform(size=(B, Ho, Wo)) >= 0.06).astype(np.uint8),
             models_dst=DST_SETS[name], params_dst=rows(DST_SETS[name], DST_ROWS), models_src=SRC_MODELS, params_src=rows(SRC_MODELS, SRC_ROWS),
             T_shared=_pose(g), T_batch=np.stack([_pose(g) for _ in range(B)]),
             src_f32=g.uniform(0.0, 5.0, size=(B, 1, Hs, Ws)).astype(np.float32), src_mask=(g.uniform(size=(B, 1, Hs, Ws)) >= 0.1).astype(np.uint8),
             src_u8=g.randint(0, 256, size=(B, 3, Hs, Ws)).astype(np.uint8))
    sd = g.uniform(2.0, 10.0, size=(B, 1, Hs, Ws)).astype(np.float32)
    h = g.uniform(size=sd.shape)
    sd[h < 0.03] = 0.0
    sd[(h >= 0.03) & (h < 0.05)] = np.nan
    sd[(h >= 0.05) & (h < 0.06)] = -2.0
    d["src_depth"] = sd
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def transform_of(c, which):
    return {"none": None, "shared": c["T_shared"], "batch": c["T_batch"]}[which]


def source_of(c, kind):
    """(src, src_mask or None, normalize, out dtype) of a KINDS entry"""
    dt, _, odt, has_mask, normalize = KINDS[kind]
    return (c["src_f32"] if dt == np.float32 else c["src_u8"]), (c["src_mask"] if has_mask else None), normalize, odt


def host_warp(exe, src, *, depth=None, points=None, params_dst=None, models_dst=None, params_src, models_src, T=None, mode="bilinear",
              padding="zeros", src_mask=None, valid_in=None, normalize=False, out_u8=False, src_depth=None, tol=0.0):
    """tests/warp_host: the fused per-pixel function on numpy inputs, after the program has checked it against the chain of the separate
    functions (exit status 3 when they differ, a sanitizer report otherwise).  Arrays are sized exactly to their contents.
    -> dict(out [B,C,Ho,Wo], valid bool [B,Ho,Wo], visible bool or None, uv [B,2,Ho,Wo], proj_depth [B,Ho,Wo])"""
    geo = depth if depth is not None else points
    Bn, (Ho, Wo) = geo.shape[0], geo.shape[-2:]
    _, Cc, Hs, Ws = src.shape
    n = Ho * Wo
    u8 = src.dtype == np.uint8
    Tn = None if T is None else np.ascontiguousarray(T, np.float32).reshape(-1, 3, 4)
    blobs = [np.ascontiguousarray(src).tobytes()]
    blobs += [np.ascontiguousarray(src_mask, np.uint8).tobytes()] if src_mask is not None else []
    blobs += [np.ascontiguousarray(src_depth, np.float32).tobytes()] if src_depth is not None else []
    blobs += [np.ascontiguousarray(geo, np.float32).tobytes()]
    blobs += [np.ascontiguousarray(params_dst, np.float32).tobytes()] if depth is not None else []
    blobs += [np.ascontiguousarray(params_src, np.float32).tobytes()]
    blobs += [Tn.tobytes()] if Tn is not None else []
    blobs += [np.ascontiguousarray(valid_in, np.uint8).tobytes()] if valid_in is not None else []
    args = [MODES[mode], PADDINGS[padding], int(normalize), int(u8), int(out_u8), int(depth is not None), Bn, Cc, Ho, Wo, Hs, Ws, src.shape[0],
            0 if src_mask is None else src_mask.shape[0], 0 if src_depth is None else src_depth.shape[0], 0 if Tn is None else Tn.shape[0],
            int(valid_in is not None), tol_bits(tol)]
    args += list(models_dst) if models_dst is not None else [0] * Bn
    args += list(models_src)
    osz = 1 if out_u8 else 4
    parts = host_program.run(exe, args, blobs, [Bn * Cc * n * osz, Bn * n, Bn * n if src_depth is not None else 0, Bn * 2 * n * 4, Bn * n * 4])
    return dict(out=np.frombuffer(parts[0], np.uint8 if out_u8 else np.float32).reshape(Bn, Cc, Ho, Wo),
                valid=np.frombuffer(parts[1], np.uint8).reshape(Bn, Ho, Wo).astype(bool),
                visible=np.frombuffer(parts[2], np.uint8).reshape(Bn, Ho, Wo).astype(bool) if src_depth is not None else None,
                uv=np.frombuffer(parts[3], np.float32).reshape(Bn, 2, Ho, Wo), proj_depth=np.frombuffer(parts[4], np.float32).reshape(Bn, Ho, Wo))


def build_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "warp_host")


def points_in_front(g, n_b, Ho, Wo):
    """points in front of the camera with a tenth behind it and a few at z = 0"""
    xy = g.uniform(-1.5, 1.5, size=(n_b, 2, Ho, Wo))
    z = g.uniform(2.0, 8.0, size=(n_b, 1, Ho, Wo))
    p = np.concatenate([xy * z / 4.0, z], axis=1).astype(np.float32)
    h = g.uniform(size=(n_b, Ho, Wo))
    p[:, 2][h < 0.1] *= -1.0
    p[:, 2][(h >= 0.1) & (h < 0.12)] = 0.0
    return p


def special_case():
    """the special values: destination depth 0, negative, NaN, +inf, -inf, -0.0 and 1e-30 at the head of the first two rows of every
    image; per-image transforms of which one holds 1e30 in every entry, one -1e30 in one, one sends every point to z' = 0 and one to
    z' < 0; NaN and 0 spread over src_depth.  -> (the mixed case, depth, T [B,3,4], src_depth)"""
    c = case("mixed")
    depth = np.array(c["depth"])
    depth[:, 0, 0, 0:4] = [0.0, -3.0, np.nan, np.inf]
    depth[:, 0, 1, 0:4] = [np.inf, -np.inf, -0.0, 1e-30]
    T = np.array(c["T_batch"])
    T[1] = 1e30
    T[2, 0, 3] = -1e30
    T[3, 2, :] = [0.0, 0.0, 0.0, 0.0]                                          # z' = 0 for every pixel of image 3
    T[4, 2, :] = [0.0, 0.0, -1.0, 0.0]                                         # z' < 0 for every pixel of image 4
    sd = np.array(c["src_depth"])
    sd[:, 0, ::3, ::2] = np.nan
    sd[:, 0, 1::3, 1::2] = 0.0
    return c, depth, T, sd


def known_answer_inputs():
    """Pinhole on both sides, fx = fy = 64, cx = 32, cy = 16, a constant depth of 2 and a translation of (0.5, 0, 0): u_src = u_dst + 16
    with every intermediate exact in fp32"""
    H, W, Bn = 32, 64, 2
    g = np.random.RandomState(9301)
    row = np.zeros((Bn, 16), np.float32)
    row[:, :4] = [64.0, 64.0, 32.0, 16.0]
    T = np.array([[1.0, 0, 0, 0.5], [0, 1.0, 0, 0], [0, 0, 1.0, 0]], np.float32)
    return dict(H=H, W=W, B=Bn, rows=row, T=T, depth=np.full((Bn, 1, H, W), 2.0, np.float32),
                src=g.uniform(-4.0, 4.0, size=(Bn, 3, H, W)).astype(np.float32))


def check_known_answer(run):
    """run(T, src_depth or None, mode) -> (out, valid, visible or None) as numpy"""
    k = known_answer_inputs()
    W, src = k["W"], k["src"]
    out, valid, _ = run(k["T"], None, "nearest")
    assert np.array_equal(out[..., :W - 16].view(np.uint32), src[..., 16:].view(np.uint32)) and not out[..., W - 16:].any()
    assert valid[..., :W - 16].all() and not valid[..., W - 16:].any()
    out, valid, _ = run(k["T"], None, "bilinear")                              # exact pixel centres: the same
    assert np.array_equal(out[..., :W - 16].view(np.uint32), src[..., 16:].view(np.uint32)) and not valid[..., W - 16:].any()
    ident = np.array(k["T"])
    ident[0, 3] = 0.0
    for mode in ("nearest", "bilinear"):
        out, valid, _ = run(ident, None, mode)
        assert np.array_equal(out.view(np.uint32), src.view(np.uint32)) and valid.all()
    for const, want in ((2.0, True), (3.0, False)):                            # |3 - 2| = 1 > 0.25 * 2
        sd = np.full((k["B"], 1, k["H"], W), const, np.float32)
        out, valid, visible = run(k["T"], sd, "nearest")
        assert valid[..., :W - 16].all() and (visible[valid] == want).all() and not visible[~valid].any()


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------

def prepared(params, models):
    """a PreparedCamera on the GPU from numpy rows and model tags"""
    import torch
    from unidepth_amd import gtpoints
    return gtpoints.PreparedCamera(torch.from_numpy(np.array(params, np.float32, order="C")).cuda(), models)


def oracle(src, *, depth=None, camera=None, points=None, src_camera, transform=None, mode="bilinear", padding="zeros", src_mask=None,
           valid_in=None, normalize=False, out_dtype=None, src_depth=None, occlusion_tol=None):
    """the composition of the merged calls: (out, valid [B,1,Ho,Wo], visible [B,1,Ho,Wo] or None, uv [B,2,Ho,Wo], proj_depth [B,Ho,Wo])"""
    from unidepth_amd import reproject, unproject
    from unidepth_amd.remap import remap
    Hs, Ws = src.shape[-2:]
    if points is None:
        Bn, (Ho, Wo) = depth.shape[0], depth.shape[-2:]
        pts = unproject.unproject_camera(None, camera, depth=depth, image_shape=(Ho, Wo))
    else:
        Bn, (Ho, Wo) = points.shape[0], points.shape[-2:]
        pts = points
    uv, inside, dproj = reproject.project_camera(pts, src_camera, image_shape=(Hs, Ws), transform=transform)
    cv = inside & (dproj > 0)
    if valid_in is not None:
        cv = cv & valid_in.reshape(-1, Ho, Wo).bool()
    if points is None:
        cv = cv & (depth.reshape(Bn, Ho, Wo) > 0)
    out, valid = remap(src, uv, mode=mode, padding=padding, src_mask=src_mask, coord_valid=cv, normalize=normalize, out_dtype=out_dtype,
                       return_mask=True)
    visible = None
    if src_depth is not None:
        m = src_depth > 0
        if src_mask is not None:
            m = m & src_mask.bool()
        ds, dv = remap(src_depth, uv, mode=mode, padding=padding, src_mask=m, coord_valid=cv, normalize=True, return_mask=True)
        dp = dproj[:, None]
        visible = dv & ((ds - dp).abs() <= occlusion_tol * dp)
    return out, valid, visible, uv, dproj


def assert_same(got, want, what=""):
    host_program.assert_same(got, want, ("out", "valid", "visible", "uv", "proj_depth"), what)
