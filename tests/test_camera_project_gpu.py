"""GPU tests of the projecting side of the camera models (csrc/project.hip through ud_camera_project, csrc/splat.hip through
ud_splat_camera, unidepth_amd/reproject.py project_camera / render_depth_camera, Camera.project of unidepth_amd/cameras.py) against
the reference's own Camera.project arrays (tests/golden/camera_project.npz) at the measured bars and against the numpy fp32
restatement of tools/make_golden_camera_project.py (pinned to the reference by tests/test_camera_project_cpu.py).

The kernel tests call the C-ABI with every output inside a tests/layout_guard.py guard allocation, twice: the guard bands must keep
their bits and both calls must give the same bits.  uv is bit-equal to the restatement for Pinhole, EUCM, OPENCV and MEI and within
the model's bar for Spherical and Fisheye624 (atan2f, asinf and atanf differ between libraries); the regular points keep a margin to
every decision, so masks, cells, indices and counts are exact for every model.  Mean mode is within test_render_depth_gpu's bound
2^-25 + (2^-24 + 2^-50) |m| of the float64 mean m."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import camera_project_common as common

pytestmark = pytest.mark.gpu

ROOT = common.ROOT
cp, gp = common.cp, common.gp
_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(ROOT, "tests", "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)


def _guard(n, dtype):
    """`n` elements of `dtype` inside a guard allocation, seen as a flat tensor."""
    words = max(1, -(-n * torch.empty(0, dtype=dtype).element_size() // 4))
    g = lg.guarded(words, 1, 1, torch.float32)
    return g, g.view.reshape(-1).view(dtype)[:n]


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def _mean_bound(m):
    return 2.0 ** -25 + (2.0 ** -24 + 2.0 ** -50) * np.abs(m)


def _layout(xyz, layout):
    """rows [B,N,3] -> (device tensor, element strides) in the asked layout"""
    B, N = xyz.shape[:2]
    if layout == "planar":
        return torch.from_numpy(np.ascontiguousarray(xyz.transpose(0, 2, 1))).cuda(), (3 * N, 1, N)
    return torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), (3 * N, 3, 1)


def _project(xyz, layout, params, models, hw, T=None):
    """ud_camera_project on guarded outputs, twice -> (uv [B,N,2], inside bool [B,N], depth [B,N]) on the host"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    B, N = xyz.shape[:2]
    src, strides = _layout(xyz, layout)
    dev_p = torch.from_numpy(np.ascontiguousarray(params, np.float32)).cuda()
    dev_T = None if T is None else torch.from_numpy(np.ascontiguousarray(T, np.float32)).cuda()
    gu, uv = _guard(2 * B * N, torch.float32)
    gi, inside = _guard(B * N, torch.uint8)
    gd, depth = _guard(B * N, torch.float32)
    rows = layout == "rows"
    d = mk(_lib.UdCameraProject, xyz=src, params=dev_p, T=dev_T, uv=uv.data_ptr(), inside=inside.data_ptr(), depth=depth.data_ptr(),
           batch_stride=strides[0], point_stride=strides[1], comp_stride=strides[2], n_points=N, B=B, H=hw[0], W=hw[1],
           nT=0 if T is None else dev_T.reshape(-1, 3, 4).shape[0], uv_rows=int(rows))
    for b, m in enumerate(models):
        d.model[b] = int(m)
    outs = []
    for _ in range(2):
        check(_lib.lib.ud_camera_project(d, cur_stream()), "ud_camera_project")
        torch.cuda.synchronize()
        outs.append([_bits(t) for t in (uv, inside, depth)])
    lg.check_guards(gu, gi, gd)
    for a, b in zip(*outs):
        assert np.array_equal(a, b), "two calls gave different bits"
    uv = uv.cpu().numpy()
    uv = uv.reshape(B, N, 2) if rows else np.ascontiguousarray(uv.reshape(B, 2, N).transpose(0, 2, 1))
    got_in = inside.cpu().numpy().reshape(B, N)
    assert set(np.unique(got_in)) <= {0, 1}
    return uv, got_in.astype(bool), depth.cpu().numpy().reshape(B, N)


def _splat(clouds, layout, params, models, hw, T=None, colors=None, mode="nearest", pixel_offset=0.0, rounding="floor", depth_range=None,
           cos_limit=None, want_index=True, want_count=True):
    """ud_splat_camera on guarded outputs and a 0xA5 work buffer, twice, checked against cp.render(); clouds: a list of [n_b,3]"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    B, (H, W) = len(clouds), hw
    nearest = mode == "nearest"
    ref = cp.render(clouds, params, models, hw, T=T, mode=mode, pixel_offset=pixel_offset, rounding=rounding, depth_range=depth_range,
                    cos_limit=cos_limit, colors=colors if nearest else None)
    colors = colors if nearest else None
    want_index = want_index and nearest
    offsets = color = None
    if layout == "packed":
        n = sum(c.shape[0] for c in clouds)
        pad = np.tile(np.array([[0.0, 0.0, 0.5]], dtype=np.float32), (5, 1))       # rows behind offsets[B]: owned by no image
        src = torch.from_numpy(np.concatenate(list(clouds) + [pad])).cuda()
        color = None if colors is None else torch.from_numpy(np.concatenate(list(colors) + [np.full((5, 3), 77, dtype=colors[0].dtype)])).cuda()
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)).cuda()
        strides, n_points = (0, 3, 1), n + 5
    else:
        n_points = clouds[0].shape[0]
        assert all(c.shape[0] == n_points for c in clouds)
        src, strides = _layout(np.stack(clouds), layout)
        color = None if colors is None else _layout(np.stack(colors), layout)[0]
    dev_p = torch.from_numpy(np.ascontiguousarray(params, np.float32)).cuda()
    dev_T = None if T is None else torch.from_numpy(np.ascontiguousarray(T, np.float32)).cuda()
    f32_color = color is not None and color.dtype == torch.float32
    px = B * H * W
    gd, depth = _guard(px, torch.float32)
    gi, index = _guard(px, torch.int32)
    gn, count = _guard(px, torch.int32)
    gc, rgb = _guard(3 * px, torch.float32 if f32_color else torch.uint8)
    before = [_bits(t) for t in (depth, index, count, rgb)]
    nbytes = int(_lib.lib.ud_splat_work_bytes(B, H, W))
    work = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    flags = (_lib.UD_SPLAT_TRUNC if rounding == "trunc" else 0) | (_lib.UD_SPLAT_RANGE if depth_range is not None else 0)
    flags |= _lib.UD_SPLAT_FOV if cos_limit is not None else 0
    d = mk(_lib.UdSplatCamera, xyz=src, offsets=offsets, params=dev_p, T=dev_T, color=color, depth=depth.data_ptr(),
           index=index.data_ptr() if want_index else None, count=count.data_ptr() if want_count else None,
           rgb=rgb.data_ptr() if color is not None else None, work=work, work_bytes=nbytes, batch_stride=strides[0], point_stride=strides[1],
           comp_stride=strides[2], n_points=n_points, B=B, H=H, W=W, nT=0 if T is None else dev_T.reshape(-1, 3, 4).shape[0],
           mode=_lib.UD_SPLAT_NEAREST if nearest else _lib.UD_SPLAT_MEAN, flags=flags, color_f32=int(f32_color), pixel_offset=pixel_offset,
           dmin=0.0 if depth_range is None else depth_range[0], dmax=0.0 if depth_range is None else depth_range[1],
           cos_limit=0.0 if cos_limit is None else cos_limit)
    for b, m in enumerate(models):
        d.model[b] = int(m)
    runs = []
    for _ in range(2):                                        # the second call finds the first call's words in the work buffer
        check(_lib.lib.ud_splat_camera(d, cur_stream()), "ud_splat_camera")
        torch.cuda.synchronize()
        runs.append([_bits(t) for t in (depth, index, count, rgb)])
    lg.check_guards(gd, gi, gn, gc)
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two calls gave different bits"
    for asked, a, b in zip((True, want_index, want_count, color is not None), before, runs[1]):
        assert asked or np.array_equal(a, b), "an output that was not requested was written"
    out = {"depth": depth.cpu().numpy().reshape(B, H, W), "index": index.cpu().numpy().reshape(B, H, W) if want_index else None,
           "count": count.cpu().numpy().reshape(B, H, W) if want_count else None,
           "rgb": rgb.cpu().numpy().reshape(B, 3, H, W) if color is not None else None}
    _compare(out, ref, mode)
    return out, ref


def _compare(out, ref, mode):
    if out["count"] is not None:
        assert np.array_equal(out["count"], ref["count"])
    if mode == "nearest":
        assert np.array_equal(out["depth"].view(np.uint32), ref["depth"].view(np.uint32))
        if out["index"] is not None:
            assert np.array_equal(out["index"], ref["index"])
        if out["rgb"] is not None:
            assert out["rgb"].dtype == ref["rgb"].dtype and np.array_equal(out["rgb"].view(np.uint8), np.ascontiguousarray(ref["rgb"]).view(np.uint8))
    else:
        m = ref["depth"]
        err = np.abs(out["depth"].astype(np.float64) - m)
        print(f"mean mode: worst error / bound {float((err / _mean_bound(m)).max()):.3f}")
        assert (err <= _mean_bound(m)).all()
        assert (out["depth"][ref["count"] == 0] == 0).all()


def _regular(c):
    return [c["xyz"][b, :c["n_reg"]] for b in range(len(c["models"]))]


# ---- 1. every case, both layouts, three references --------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["planar", "rows"])
@pytest.mark.parametrize("name", list(cp.CASES))
def test_project_cases(name, layout):
    c, g, bars = common.case(name), common.golden(), common.bars()
    uv, inside, depth = _project(c["xyz"], layout, c["params"], c["models"], (c["H"], c["W"]))
    w = common.assert_uv(uv, c, bars, f"{name} {layout}", ref=common.rows_of(g[name + ".uv"]))
    assert np.array_equal(inside, c["in32"]), "the in-image test differs from the restatement"
    assert common.same_bits(depth, c["d32"])
    print(f"{name} {layout}: worst error / bar {w:.3f}")


@pytest.mark.parametrize("name", list(cp.CASES))
def test_class_methods_return_the_references_masks(name):
    """Camera.project / get_projection_mask of every class, member by member as the reference's BatchCamera calls them, and of the
    BatchCamera in one launch: the reference's uv at the bars, its mask exactly on the regular points (Pinhole's inverted, Spherical's
    None), the restatement's on every point"""
    from unidepth_amd import cameras
    c, g, bars = common.case(name), common.golden(), common.bars()
    H, W, n = c["H"], c["W"], c["n_reg"]
    pts = torch.from_numpy(cp.planar(c["xyz"], H, W)).cuda()
    ref_uv = common.rows_of(g[name + ".uv"])
    members = [gp.make_camera(cameras, m, r) for m, r in zip(c["models"], c["params"])]
    single = []
    for b, (m, cam) in enumerate(zip(c["models"], members)):
        before = cam.params.clone()
        uv = cam.project(pts[b:b + 1])
        assert uv.shape == (1, 2, H, W) and uv.dtype == torch.float32 and torch.equal(cam.params, before)
        single.append(uv)
        mask, want = cam.get_projection_mask(), g[name + ".mask"][b]
        if m == cp.SPHERICAL:
            assert mask is None and (want == 2).all()
            continue
        assert mask.dtype == torch.bool and mask.shape == (1, 1, H, W)
        got = mask.cpu().numpy().reshape(-1)
        assert np.array_equal(got[:n], want.reshape(-1)[:n].astype(bool)), "the reference's mask on the regular points"
        assert np.array_equal(got, cp.class_mask(m, c["in32"][b]).astype(bool)), "the restatement's mask on every point"
    uv1 = torch.cat(single)
    common.assert_uv(common.rows_of(uv1.cpu().numpy()), c, bars, name, ref=ref_uv)
    batch = cameras.BatchCamera(members)
    uvb = batch.project(pts)
    assert torch.equal(uvb.view(torch.int32), uv1.view(torch.int32)), "one launch for the batch gives the members' bits"
    mb = batch.get_projection_mask()
    assert mb.shape == (len(members), 1, H, W) and mb.dtype == torch.bool
    for b, m in enumerate(c["models"]):
        want = c["in32"][b] if m == cp.SPHERICAL else cp.class_mask(m, c["in32"][b]).astype(bool)
        assert np.array_equal(mb[b].cpu().numpy().reshape(-1), want)


# ---- 2. chunk boundaries and packed clouds ---------------------------------------------------------------------------------------

def _tiled(name, n):
    """n regular points per image of a case, repeated as needed, each repetition a little farther away so depths differ"""
    c = common.case(name)
    reps = -(-n // c["n_reg"])
    clouds = []
    for b in range(len(c["models"])):
        r = c["xyz"][b, :c["n_reg"]]
        clouds.append(np.concatenate([r * np.float32(1.0 + 0.125 * k) for k in range(reps)])[:n].copy())
    return c, clouds


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
def test_rows_at_the_chunk_boundaries(n):
    from unidepth_amd import project_camera, render_depth_camera
    c, clouds = _tiled("mixed_5x7_b6", n)
    hw = (c["H"], c["W"])
    xyz = np.stack(clouds)
    for layout in ("rows", "planar"):
        uv, inside, depth = _project(xyz, layout, c["params"], c["models"], hw)
        r_uv, r_in, r_d = cp.project(xyz, c["params"], c["models"], hw)
        cc = dict(models=c["models"], uv32=r_uv, uv64=cp.project(xyz, c["params"], c["models"], hw, None, np.float64)[0], n_reg=n)
        common.assert_uv(uv, cc, common.bars(), f"n={n} {layout}")
        assert np.array_equal(inside, r_in) and common.same_bits(depth, r_d)
        _splat(clouds, layout, c["params"], c["models"], hw)
    _splat(clouds, "rows", c["params"], c["models"], hw, mode="mean")
    # the Python surface on the same rows
    from unidepth_amd import cameras
    cam = gp.case_camera(cameras, "mixed_5x7_b6")
    t = torch.from_numpy(xyz).cuda()
    uv, inside, depth = project_camera(t, cam, image_shape=hw)
    assert uv.shape == (6, n, 2) and inside.shape == (6, n) and inside.dtype == torch.bool and depth.shape == (6, n)
    assert np.array_equal(inside.cpu().numpy(), r_in) and common.same_bits(depth.cpu().numpy(), r_d)
    view = render_depth_camera(t, cam, hw, return_index=True, return_count=True)
    ref = cp.render(clouds, c["params"], c["models"], hw)
    _compare({"depth": view.depth[:, 0].cpu().numpy(), "index": view.index.cpu().numpy(), "count": view.count.cpu().numpy(), "rgb": None}, ref, "nearest")


def test_packed_point_cloud():
    from unidepth_amd import PointCloud, cameras, render_depth_camera
    c = common.case("mixed_37x53_b6")
    hw = (c["H"], c["W"])
    sizes = [1500, 0, 1024, 1025, 7, 1946]
    clouds = [c["xyz"][b, :k].copy() for b, k in enumerate(sizes)]
    g = torch.Generator().manual_seed(11)
    colors = [torch.randint(0, 256, (k, 3), generator=g, dtype=torch.uint8).numpy() for k in sizes]
    _splat(clouds, "packed", c["params"], c["models"], hw, colors=colors)
    _splat(clouds, "packed", c["params"], c["models"], hw, mode="mean")
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64).cuda()
    cloud = PointCloud(torch.from_numpy(np.concatenate(clouds)).cuda(), torch.from_numpy(np.concatenate(colors)).cuda(), None,
                       torch.tensor(sizes, dtype=torch.int64).cuda(), offsets)
    view = render_depth_camera(cloud, gp.case_camera(cameras, "mixed_37x53_b6"), hw, return_index=True, return_count=True)
    ref = cp.render(clouds, c["params"], c["models"], hw, colors=colors)
    _compare({"depth": view.depth[:, 0].cpu().numpy(), "index": view.index.cpu().numpy(), "count": view.count.cpu().numpy(),
              "rgb": view.rgb.cpu().numpy()}, ref, "nearest")


# ---- 3. render_depth_camera -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(cp.CASES))
def test_render_cases(name):
    c = common.case(name)
    hw = (c["H"], c["W"])
    clouds = _regular(c)
    g = torch.Generator().manual_seed(23)
    colors = [torch.randint(0, 256, (len(p), 3), generator=g, dtype=torch.uint8).numpy() for p in clouds]
    out, ref = _splat(clouds, "rows", c["params"], c["models"], hw, colors=colors)
    assert (ref["index"] >= 0).any() and any(not k.all() for k in ref["kept"]), "the case must fill pixels and drop points"
    _splat(clouds, "planar", c["params"], c["models"], hw, pixel_offset=0.5, rounding="trunc", want_index=False, want_count=False)
    _splat(clouds, "rows", c["params"], c["models"], hw, mode="mean")
    _, near = _splat(clouds, "rows", c["params"], c["models"], hw, depth_range=(1.0, 3.0))
    assert near["count"].sum() < ref["count"].sum()
    _, cone = _splat(clouds, "planar", c["params"], c["models"], hw, cos_limit=math.cos(0.35))
    assert cone["count"].sum() < ref["count"].sum()


def test_render_depth_camera_arguments():
    """the Python surface: float colours, max_angle (the cosine is taken on the host), depth_range, a shared workspace, a transform"""
    from unidepth_amd import _lib, cameras, render_depth_camera
    name = "mixed_37x53_b6"
    c = common.case(name)
    hw = (c["H"], c["W"])
    clouds = _regular(c)
    cam = gp.case_camera(cameras, name)
    t = torch.from_numpy(np.stack(clouds)).cuda()
    g = torch.Generator().manual_seed(29)
    img = torch.rand(t.shape, generator=g)
    work = torch.empty(int(_lib.lib.ud_splat_work_bytes(6, *hw)), dtype=torch.uint8, device="cuda")
    T = np.tile(np.eye(4, dtype=np.float32)[:3], (6, 1, 1))
    T[:, :, 3] = np.linspace(-0.05, 0.05, 18, dtype=np.float32).reshape(6, 3)
    for kw, rkw in ((dict(image=img.cuda(), return_index=True, return_count=True), dict(colors=list(img.numpy()))),
                    (dict(max_angle=0.35, return_index=True, return_count=True), dict(cos_limit=math.cos(0.35))),
                    (dict(depth_range=(1.0, 3.0), workspace=work, return_count=True), dict(depth_range=(1.0, 3.0))),
                    (dict(transform=torch.from_numpy(T).cuda(), return_index=True, return_count=True), dict(T=T)),
                    (dict(mode="mean", return_count=True), dict(mode="mean"))):
        view = render_depth_camera(t, cam, hw, **kw)
        ref = cp.render(clouds, c["params"], c["models"], hw, **rkw)
        _compare({"depth": view.depth[:, 0].cpu().numpy(), "index": None if view.index is None else view.index.cpu().numpy(),
                  "count": view.count.cpu().numpy(), "rgb": None if view.rgb is None else view.rgb.cpu().numpy()}, ref, kw.get("mode", "nearest"))


# ---- 4. Pinhole equivalence -------------------------------------------------------------------------------------------------------

def test_pinhole_camera_equals_the_matrix_path_bitwise():
    from unidepth_amd import cameras, render_depth, render_depth_camera
    hw = (37, 53)
    g = torch.Generator().manual_seed(31)
    B, n = 3, 5000
    z = 0.01 + 6.0 * torch.rand(B, n, generator=g)
    pts = torch.stack([(torch.rand(B, n, generator=g) - 0.5) * 1.4 * z, (torch.rand(B, n, generator=g) - 0.5) * 1.0 * z, z], dim=2)
    pts[0, 0, 2] = 0.01
    K = torch.tensor([[[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]], [[40.0, 0, 25.5], [0, 41.0, 18.5], [0, 0, 1]], [[62.0, 0, 27.0], [0, 60.0, 17.0], [0, 0, 1]]])
    img = torch.randint(0, 256, (B, n, 3), generator=g, dtype=torch.uint8)
    for kw in (dict(image=img.cuda(), return_index=True, return_count=True), dict(mode="mean", return_count=True),
               dict(pixel_offset=0.5, rounding="trunc", depth_range=(0.5, 4.0), return_index=True)):
        a = render_depth(pts.cuda(), K.cuda(), hw, **kw)
        for cam in (cameras.Pinhole(K), K.cuda()):
            b = render_depth_camera(pts.cuda(), cam, hw, **kw)
            for x, y in zip((a.depth, a.rgb, a.index, a.count), (b.depth, b.rgb, b.index, b.count)):
                assert (x is None) == (y is None) and (x is None or np.array_equal(_bits(x), _bits(y)))
    assert int((a.index >= 0).sum()) > 500


# ---- 5. round trip without the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cp.roundtrip_cases()))
def test_round_trip_through_gt_points(name):
    """depth -> gt_points -> render_depth_camera with the same camera and pixel_offset 0: every pixel gets its own point back, with the
    depth it started from to within the bar gt_points itself is held to (Spherical: the distance)"""
    import gt_points_common as gcommon
    from unidepth_amd import cameras, gt_points, render_depth_camera
    depth = cp.roundtrip_cases()[name]
    B, _, H, W = depth.shape
    _, params, models = gp.case_rows(name)
    cam = gp.case_camera(cameras, name)
    d = torch.from_numpy(depth).cuda()
    pts = gt_points(d, cam)
    view = render_depth_camera(pts, cam, (H, W), pixel_offset=0.0, return_index=True, return_count=True)
    own = torch.arange(H * W, dtype=torch.int32, device="cuda").reshape(1, H, W).expand(B, H, W)
    assert torch.equal(view.index, own) and bool((view.count == 1).all())
    bars = gcommon.bars()
    got = view.depth.cpu().numpy().astype(np.float64)
    for b, m in enumerate(models):
        e = np.abs(got[b] - depth[b]) / np.maximum(np.abs(depth[b]), 1e-4 * np.maximum(np.abs(depth[b]), 1.0))
        assert e.max() <= bars[m], f"{name}: image {b} ({cp.MODEL_NAMES[m]}) depth error {e.max():.3e} above the bar {bars[m]:.3e}"


# ---- 6. six different members, a transform per image ------------------------------------------------------------------------------

def test_batch_camera_with_a_transform_per_image():
    from unidepth_amd import cameras, project_camera
    name = "mixed_37x53_b6"
    c = common.case(name)
    hw = (c["H"], c["W"])
    assert sorted(c["models"]) == sorted(cp.MODEL_NAMES)
    xyz = np.stack(_regular(c))
    ang = np.linspace(-0.02, 0.02, 6)
    T = np.zeros((6, 3, 4), np.float32)
    for b, a in enumerate(ang):
        T[b] = np.array([[math.cos(a), 0, math.sin(a), 0.01 * b], [0, 1, 0, -0.02], [-math.sin(a), 0, math.cos(a), 0.03]], np.float32)
    r_uv, r_in, r_d = cp.project(xyz, c["params"], c["models"], hw, T)
    cc = dict(models=c["models"], uv32=r_uv, uv64=cp.project(xyz, c["params"], c["models"], hw, T, np.float64)[0], n_reg=xyz.shape[1])
    for layout in ("rows", "planar"):
        uv, inside, depth = _project(xyz, layout, c["params"], c["models"], hw, T=T)
        common.assert_uv(uv, cc, common.bars(), f"transform {layout}")
        assert common.same_bits(depth, r_d)
        # a transformed point may come within a last bit of the border: the mask is compared where the fp64 restatement is clear of it
        uv64 = cc["uv64"]
        clear = (np.abs(uv64 * 2 - np.rint(uv64 * 2)) > 2 * cp.MARGIN).all(axis=2)
        assert np.array_equal(inside[clear], r_in[clear]) and clear.mean() > 0.9
    one = T[2:3]
    uv, _, _ = _project(xyz, "rows", c["params"], c["models"], hw, T=one)
    common.assert_uv(uv, dict(cc, uv32=cp.project(xyz, c["params"], c["models"], hw, one)[0],
                              uv64=cp.project(xyz, c["params"], c["models"], hw, one, np.float64)[0]), common.bars(), "one transform")
    T4 = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    T4[:, :3] = T
    uv, inside, depth = project_camera(torch.from_numpy(xyz).cuda(), gp.case_camera(cameras, name), hw, transform=torch.from_numpy(T4).cuda())
    common.assert_uv(uv.cpu().numpy(), cc, common.bars(), "project_camera with a transform")
    assert common.same_bits(depth.cpu().numpy(), r_d)


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------

def test_graph_capture_with_a_prepared_camera():
    from unidepth_amd import _lib, cameras, prepare_camera, project_camera, render_depth_camera
    name = "mixed_5x7_b6"
    c = common.case(name)
    hw = (c["H"], c["W"])
    first = np.stack(_regular(c))
    second = np.ascontiguousarray(first[:, ::-1] * np.float32(1.25))
    prepared = prepare_camera(gp.case_camera(cameras, name), 6, "cuda")
    static = torch.from_numpy(first).cuda()
    work = torch.empty(int(_lib.lib.ud_splat_work_bytes(6, *hw)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                # warm-up outside the capture
        project_camera(static, prepared, hw)
        render_depth_camera(static, prepared, hw, return_index=True, workspace=work)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        uv, inside, depth = project_camera(static, prepared, hw)
        view = render_depth_camera(static, prepared, hw, return_index=True, return_count=True, workspace=work)
    for pts in (first, second, first):
        static.copy_(torch.from_numpy(pts).cuda())
        graph.replay()
        torch.cuda.synchronize()
        r_uv, r_in, r_d = cp.project(pts, c["params"], c["models"], hw)
        cc = dict(models=c["models"], uv32=r_uv, uv64=cp.project(pts, c["params"], c["models"], hw, None, np.float64)[0], n_reg=pts.shape[1])
        common.assert_uv(uv.cpu().numpy(), cc, common.bars(), "replay")
        assert common.same_bits(depth.cpu().numpy(), r_d)
        ref = cp.render(list(pts), c["params"], c["models"], hw)
        if pts is first:                                      # the scaled points of `second` have no margin to the cell borders
            assert np.array_equal(inside.cpu().numpy(), r_in)
            _compare({"depth": view.depth[:, 0].cpu().numpy(), "index": view.index.cpu().numpy(), "count": view.count.cpu().numpy(), "rgb": None}, ref, "nearest")
        else:
            assert int((view.index >= 0).sum()) > 0 and not np.array_equal(view.index.cpu().numpy(), cp.render(list(first), c["params"], c["models"], hw)["index"])
