"""GPU parity of unproject_camera / get_rays (unidepth_amd/unproject.py -> ud_camera_unproject, csrc/unproject.hip) against the numpy
fp32 restatement of tools/make_golden_unproject.py (bit for bit where the arithmetic has no libm call), the reference's own
Camera.unproject arrays and masks (tests/golden/unproject.npz) at the measured bars, and gt_points (the identity grid with a depth);
partial waves and several workgroups per image, the three output forms, layouts, guarded outputs, graph replay and the round trip through
project_camera.  Every point of every case is compared: none is excluded.  Shared helpers: tests/unproject_common.py.

Every case runs once per process and form through the C-ABI with guarded buffers (_gpu_case) and is shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import layout_guard as lg
import unproject_common as common

up, gp, cp = common.up, common.gp, common.cp
pytestmark = pytest.mark.gpu

# Models whose arithmetic has no libm call (only +, -, *, /, sqrt, all correctly rounded on both sides): bit-equal to the numpy fp32
# restatement.  Spherical (sinf / cosf) and Fisheye624 (tanf) differ from numpy's functions in the last bits and keep the bar.
EXACT_MODELS = (up.PINHOLE, up.EUCM, up.OPENCV, up.MEI)


def _guard(n, dtype):
    """`n` elements of `dtype` inside a guard allocation, seen as a flat tensor."""
    words = max(1, -(-n * torch.empty(0, dtype=dtype).element_size() // 4))
    g = lg.guarded(words, 1, 1, torch.float32)
    return g, g.view.reshape(-1).view(dtype)[:n]


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _raw_call(uv, params, models, form="raw", depth=None, src="rows", out_rows=True, hw=(1, 1), want_mask=True):
    """ud_camera_unproject with rays, valid and work inside sentinel-filled allocations, twice.  uv: numpy [B,N,2] / [1,N,2] (shared:
    batch_stride 0), or None for the identity grid of hw; src: the layout uv is handed over in.  Returns (rays [B,N,3], mask bool [B,N])
    on the host after checking the guards."""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    B = len(models)
    N = hw[0] * hw[1] if uv is None else uv.shape[1]
    dev_uv, strides = None, (0, 1, 1)
    if uv is not None:
        if src == "rows":
            dev_uv, strides = torch.from_numpy(np.ascontiguousarray(uv)).cuda(), (2 * N, 2, 1)
        else:
            dev_uv, strides = torch.from_numpy(np.ascontiguousarray(uv.transpose(0, 2, 1))).cuda(), (2 * N, 1, N)
        if uv.shape[0] == 1:
            strides = (0,) + strides[1:]
    dev_p = torch.from_numpy(np.ascontiguousarray(params, np.float32)).cuda()
    dev_d = None if form != "depth" else torch.from_numpy(np.ascontiguousarray(depth, np.float32).reshape(B, N)).cuda()
    gr, rays = _guard(3 * B * N, torch.float32)
    gv, valid = _guard(B * N, torch.uint8)
    guards = [gr, gv]
    n_iter = sum(m in up.ITERATIVE for m in models)
    nbytes = int(_lib.lib.ud_camera_unproject_work_bytes(B, n_iter))
    work = None
    if nbytes:
        assert nbytes % 16 == 0
        gw = lg.guarded(1, nbytes // 4, nbytes // 4, torch.float32, pre_rows=4, post_rows=4)
        assert gw.ptr() % 16 == 0
        work = gw.ptr()
        guards.append(gw)
    d = mk(_lib.UdCameraUnproject, uv=dev_uv, params=dev_p, depth=dev_d, rays=rays.data_ptr(), valid=valid.data_ptr() if want_mask else None,
           work=work, work_bytes=nbytes, batch_stride=strides[0], point_stride=strides[1], comp_stride=strides[2], n_points=N, B=B, H=hw[0],
           W=hw[1], normalize=int(form == "normalize"), rays_rows=int(out_rows))
    for b, m in enumerate(models):
        d.model[b] = int(m)
    outs = []
    for _ in range(2):
        check(_lib.lib.ud_camera_unproject(d, cur_stream()), "ud_camera_unproject")
        torch.cuda.synchronize()
        outs.append((rays.cpu().numpy().copy(), valid.cpu().numpy().copy()))
    lg.check_guards(*guards)
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)), "two calls gave different bits"
    got = outs[0][0].reshape(B, N, 3) if out_rows else np.ascontiguousarray(outs[0][0].reshape(B, 3, N).transpose(0, 2, 1))
    if not want_mask:
        assert (gv.view.reshape(-1).view(torch.int32) == lg.SENTINEL[torch.float32]).all()       # an absent mask is not written
        return got, None
    assert np.array_equal(outs[0][1], outs[1][1]) and set(np.unique(outs[0][1])) <= {0, 1}
    return got, outs[0][1].reshape(B, N).astype(bool)


@functools.lru_cache(maxsize=None)
def _gpu_case(name, form):
    c = common.case(name)
    return _raw_call(c["uv"], c["params"], c["models"], form, c["depth"])


def _assert_matches_restatement(rays, want, truth, models, what):
    """bit for bit for the models without a libm call, within the bar for the others; NaN and infinities in the same places"""
    assert common.same_specials(rays, want), f"{what}: NaN / infinities differ"
    bars = common.bars()
    for b, m in enumerate(models):
        if m in EXACT_MODELS:
            assert common.same_bits(np.ascontiguousarray(rays[b]), np.ascontiguousarray(want[b])), \
                f"{what}: image {b} ({up.MODEL_NAMES[m]}) is not bit-equal to the restatement"
    if truth is not None:
        common.assert_within_bars(rays, want, truth, models, bars, what)


def _camera(name):
    """the camera of a case from unidepth_amd.cameras' classes: the single camera of a broadcast case, else a BatchCamera"""
    from unidepth_amd import cameras
    c = common.case(name)
    if len(gp.CASES[up.base_case(name)][2]) == 1:
        return gp.make_camera(cameras, c["models"][0], c["params"][0])
    return cameras.BatchCamera([gp.make_camera(cameras, m, r) for m, r in zip(c["models"], c["params"])])


@pytest.mark.parametrize("name", list(up.CASES))
def test_case_against_restatement_and_reference(name):
    """every point of every case, the three forms: the fp32 restatement (bit for bit for Pinhole, EUCM, OPENCV, MEI; the bar for
    Spherical and Fisheye624), the reference's output and masks at the measured bars, guards intact; the Python surface gives the same bits"""
    from unidepth_amd import unproject
    c, g = common.case(name), common.golden()
    H, W = common.shape(name)
    for which in common.FORMS:
        rays, mask = _gpu_case(name, which)                     # raises if a guard element of rays, valid or work was rewritten
        _assert_matches_restatement(rays, common.form(c, which), c["r64"] if which == "raw" else None, c["models"], f"{name} {which}")
        assert np.array_equal(mask, c["mask"]), f"{name} {which}: mask"
        if which != "raw":                                      # the other forms of the libm models: the bar with the form's own fp64 value
            kw = dict(normalize=True) if which == "normalize" else dict(depth=c["depth"])
            t64 = up.unproject(c["uv"], c["params"], c["models"], np.float64, **kw)[0]
            if which == "depth":                                # gt_points' measure: the floor scales with the depth
                e = gp.error_ratio(planar64(rays - common.form(c, which), H, W), planar64(t64, H, W), c["depth"].reshape(len(c["models"]), 1, H, W))
                for b, m in enumerate(c["models"]):
                    assert float(e[b].max()) <= common.bars()[m], (name, which, b, float(e[b].max()))
            else:
                common.assert_within_bars(rays, common.form(c, which), t64, c["models"], common.bars(), f"{name} {which}")
    rays, mask = _gpu_case(name, "raw")
    w = common.assert_within_bars(rays, g[name + ".out"], c["r64"], c["models"], common.bars(), f"{name} vs reference")
    for b, m in enumerate(c["models"]):
        assert np.array_equal(g[name + ".mask"][b], up.class_mask(m, mask[b])), (name, b)
    print(f"{name}: {w:.3f} of the bar against the reference")
    cam = _camera(name)
    uv_rows = torch.from_numpy(c["uv"]).cuda()
    uv_planar = torch.from_numpy(up.planar(c["uv"], H, W)).cuda()
    for which in common.FORMS:
        kw = dict(normalize=True) if which == "normalize" else dict(depth=torch.from_numpy(c["depth"]).cuda()) if which == "depth" else {}
        want, want_mask = _gpu_case(name, which)
        got, got_mask = unproject.unproject_camera(uv_rows, cam, return_mask=True, **kw)
        assert got.shape == c["uv"].shape[:2] + (3,) and got_mask.shape == c["uv"].shape[:2] and got_mask.dtype == torch.bool
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(got_mask.cpu().numpy(), want_mask)
        if which == "depth":
            kw = dict(depth=torch.from_numpy(c["depth"]).cuda().reshape(-1, 1, H, W))
        got, got_mask = unproject.unproject_camera(uv_planar, cam, return_mask=True, **kw)
        assert got.shape == (len(c["models"]), 3, H, W) and got_mask.shape == (len(c["models"]), 1, H, W)
        assert np.array_equal(up.rows(got.cpu().numpy()).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got_mask.cpu().numpy().reshape(want_mask.shape), want_mask)
        assert torch.equal(_ibits(unproject.unproject_camera(uv_planar, cam, **kw)), _ibits(got))


def planar64(rws, H, W):
    return up.planar(rws.astype(np.float64), H, W)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 1961])
def test_point_counts(n):
    """the first n points of every image: 63 - 65 are partial waves inside the wave reduction, 257 several waves meeting in the
    workgroup's reduction, 1025 and 1961 the maxima of two workgroups (1024 threads each) meeting in one atomicMax.  The iteration
    counts follow the subset (the restatement's, over the same points)."""
    for name in ("mixed_37x53_b6", "opencv_37x53_b2_iters"):
        c = common.case(name)
        uv, depth = np.ascontiguousarray(c["uv"][:, :n]), np.ascontiguousarray(c["depth"][:, :n])
        for which in common.FORMS:
            kw = dict(normalize=True) if which == "normalize" else dict(depth=depth) if which == "depth" else {}
            info = {}
            want, want_mask = up.unproject(uv, c["params"], c["models"], np.float32, info, **kw)
            for src, out_rows in (("rows", True), ("planar", False)):
                rays, mask = _raw_call(uv, c["params"], c["models"], which, depth, src=src, out_rows=out_rows)
                _assert_matches_restatement(rays, want, None, c["models"], f"{name} n={n} {which} {src}")
                assert np.array_equal(mask, want_mask)
        if n == 1961 and name == "opencv_37x53_b2_iters":
            assert info["steps"] == c["info"]["steps"] and info["steps"][0] < info["steps"][1]


def test_early_exit_is_per_image():
    """iterative members at non-adjacent positions of the mixed batch, and the weakly distorted OPENCV image alone, beside the strongly
    distorted one and with the two in the other order: the same bits.  One shared row of maxima would keep the weak image iterating."""
    c = common.case("mixed_37x53_b6")
    it = [b for b, m in enumerate(c["models"]) if m in up.ITERATIVE]
    assert it == [0, 3]
    whole = _gpu_case("mixed_37x53_b6", "raw")[0]
    for b in it:
        alone = _raw_call(c["uv"][b:b + 1], c["params"][b:b + 1], [c["models"][b]])[0]
        assert np.array_equal(alone[0].view(np.uint32), whole[b].view(np.uint32))
    c = common.case("opencv_37x53_b2_iters")
    assert c["info"]["steps"][0] < c["info"]["steps"][1]
    both = _gpu_case("opencv_37x53_b2_iters", "raw")[0]
    swapped = _raw_call(c["uv"][::-1].copy(), c["params"][::-1].copy(), c["models"][::-1])[0]
    assert np.array_equal(swapped[::-1].view(np.uint32), both.view(np.uint32))


def test_broadcast_camera_and_shared_coordinates():
    """one iterative camera applied to every image; one coordinate set (batch_stride = 0) shared by every image of a mixed batch, where
    each iterative image still leaves its loop on its own"""
    from unidepth_amd import cameras, unproject
    name = "broadcast_opencv_9x29_b3"
    c = common.case(name)
    cam = _camera(name)
    assert isinstance(cam, cameras.OPENCV)
    uv = torch.from_numpy(c["uv"]).cuda()
    whole = unproject.unproject_camera(uv, cam)
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), _gpu_case(name, "raw")[0].view(np.uint32))
    for b in range(3):
        assert torch.equal(_ibits(unproject.unproject_camera(uv[b:b + 1], cam)), _ibits(whole[b:b + 1]))
    name = "mixed_37x53_b6"
    c = common.case(name)
    shared = c["uv"][2:3]                                       # the MEI image's set (with its NaN coordinate) for every image
    info = {}
    want, want_mask = up.unproject(shared, c["params"], c["models"], np.float32, info)
    assert info["steps"][0] == info["steps"][3] == 10           # the NaN keeps both iterative images in their loops
    shared = np.ascontiguousarray(shared[:, :-1])
    want, want_mask = up.unproject(shared, c["params"], c["models"], np.float32, info)
    for src in ("rows", "planar"):
        rays, mask = _raw_call(shared, c["params"], c["models"], src=src)
        _assert_matches_restatement(rays, want, None, c["models"], f"shared {src}")
        assert np.array_equal(mask, want_mask)
    got = unproject.unproject_camera(torch.from_numpy(shared).cuda(), _camera(name))
    assert got.shape == (6, shared.shape[1], 3) and np.array_equal(got.cpu().numpy().view(np.uint32), rays.view(np.uint32))


def _grid(H, W):
    u, v = np.meshgrid(np.arange(W, dtype=np.float32) + np.float32(0.5), np.arange(H, dtype=np.float32) + np.float32(0.5))
    return np.stack([u.ravel(), v.ravel()], axis=1)[None]


@pytest.mark.parametrize("name", list(gp.CASES))
def test_identity_grid(name):
    """uv = None is the grid of pixel centres passed explicitly, bit for bit, in every form; with a depth it is gt_points, bit for bit"""
    from unidepth_amd import cameras, gtpoints, unproject
    depth, params, models = gp.case_rows(name)
    B, _, H, W = depth.shape
    grid = _grid(H, W)
    for which in common.FORMS:
        ident, imask = _raw_call(None, params, models, which, depth, hw=(H, W), out_rows=False)
        expl, emask = _raw_call(grid, params, models, which, depth, src="planar", out_rows=False)
        assert np.array_equal(ident.view(np.uint32), expl.view(np.uint32)) and np.array_equal(imask, emask), (name, which)
    cam = gp.case_camera(cameras, name)
    d = torch.from_numpy(depth).cuda()
    pts = gtpoints.gt_points(d, cam)
    got = unproject.unproject_camera(None, cam, depth=d, image_shape=(H, W))
    assert got.shape == pts.shape and torch.equal(_ibits(got), _ibits(pts)), f"{name}: the identity grid with a depth is not gt_points"
    assert np.array_equal(up.rows(got.cpu().numpy()).view(np.uint32), ident.view(np.uint32))


def test_get_rays_and_camera_methods():
    """get_rays on every class and a BatchCamera: unproject at the pixel centres, normalised; Camera.unproject with the reference's masks"""
    from unidepth_amd import cameras, unproject
    name = "mixed_5x7_b6"
    depth, params, models = gp.case_rows(name)
    H, W = depth.shape[-2:]
    batch = gp.case_camera(cameras, name)
    want = up.planar(_raw_call(None, params, models, "normalize", hw=(H, W))[0], H, W)
    for shapes in ((6, H, W), (H, W)):
        got = batch.get_rays(shapes)
        assert got.shape == (6, 3, H, W) and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(_ibits(unproject.get_rays(batch, (H, W))), _ibits(got))
    n = torch.linalg.vector_norm(got.double(), dim=1)
    assert bool(((n - 1).abs() < 1e-6).all())
    uv = torch.from_numpy(up.planar(_grid(H, W), H, W)).cuda()
    raw = unproject.unproject_camera(uv, batch, return_mask=True)
    assert batch.unprojection_mask is None
    assert torch.equal(_ibits(batch.unproject(uv)), _ibits(raw[0])) and torch.equal(batch.unprojection_mask, raw[1])      # batch-1 uv: every member
    for b, member in enumerate(batch.cameras):
        assert type(member).__name__ == up.MODEL_NAMES[models[b]]
        one = member.get_rays((1, H, W))
        assert np.array_equal(one.cpu().numpy().view(np.uint32), want[b:b + 1].view(np.uint32))
        three = member.get_rays((3, H, W))                      # one camera, three images
        assert three.shape == (3, 3, H, W) and all(torch.equal(_ibits(three[k]), _ibits(one[0])) for k in range(3))
        assert torch.equal(_ibits(member.unproject(uv)), _ibits(raw[0][b:b + 1]))
        if models[b] in (up.PINHOLE, up.EUCM):
            assert torch.equal(member.unprojection_mask, raw[1][b:b + 1]) and member.unprojection_mask.shape == (1, 1, H, W)
        else:
            assert member.unprojection_mask is None
    # a stand-in for a reference class (matched by class name and .params) and an intrinsics tensor
    standin = type("EUCM", (), {})()
    standin.params = batch.cameras[1].params.clone()
    assert torch.equal(_ibits(unproject.get_rays(standin, (H, W))), _ibits(got[1:2]))
    K = batch.cameras[0].K
    for Kt in (K, K.cuda(), K[0]):
        assert torch.equal(_ibits(unproject.get_rays(Kt, (1, H, W))), _ibits(got[0:1]))
    # an EUCM camera whose mask has both values, through the class
    c = common.case("eucm_9x29_b2")
    cam = cameras.EUCM(torch.from_numpy(c["params"][:, :6]))
    cam.unproject(torch.from_numpy(c["uv"]).cuda())
    assert np.array_equal(cam.unprojection_mask.cpu().numpy(), c["mask"]) and not c["mask"].all() and c["mask"].any()


def test_input_layouts_and_dtypes():
    """offset and strided views and other float dtypes are made contiguous fp32 by the wrapper: the same bits as the plain call"""
    from unidepth_amd import unproject
    name = "mixed_37x53_b6"
    c = common.case(name)
    H, W = common.shape(name)
    cam = _camera(name)
    rows = torch.from_numpy(c["uv"]).cuda()
    planar = torch.from_numpy(up.planar(c["uv"], H, W)).cuda()
    want_rows = torch.from_numpy(_gpu_case(name, "raw")[0]).cuda()
    want_planar = unproject.unproject_camera(planar, cam)
    assert torch.equal(_ibits(want_planar.reshape(6, 3, -1).transpose(1, 2)), _ibits(want_rows))
    t = planar.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)                          # a transposed view of the same values
    assert not t.is_contiguous() and torch.equal(_ibits(unproject.unproject_camera(t, cam)), _ibits(want_planar))
    wide = torch.full((6, 2, H, W + 7), 3.0, device="cuda")
    wide[..., 4:4 + W] = planar
    assert torch.equal(_ibits(unproject.unproject_camera(wide[..., 4:4 + W], cam)), _ibits(want_planar))      # a column window
    packed = torch.full((6, H * W, 5), -1.0, device="cuda")
    packed[..., 1:3] = rows
    assert torch.equal(_ibits(unproject.unproject_camera(packed[..., 1:3], cam)), _ibits(want_rows))          # two columns of wider rows
    flat = torch.zeros(6 * H * W * 2 + 3, device="cuda")
    flat[3:] = rows.reshape(-1)
    assert torch.equal(_ibits(unproject.unproject_camera(flat[3:].view(6, H * W, 2), cam)), _ibits(want_rows))   # an offset of 12 bytes
    assert torch.equal(_ibits(unproject.unproject_camera(rows.double(), cam)), _ibits(want_rows))             # fp64 of fp32 values converts back
    h = rows.half()
    assert torch.equal(_ibits(unproject.unproject_camera(h, cam)), _ibits(unproject.unproject_camera(h.float(), cam)))
    d = torch.from_numpy(c["depth"]).cuda()
    want_d = torch.from_numpy(_gpu_case(name, "depth")[0]).cuda()
    assert torch.equal(_ibits(unproject.unproject_camera(rows, cam, depth=d.double())), _ibits(want_d))
    dw = torch.zeros(6, H * W + 5, device="cuda")
    dw[:, 2:2 + H * W] = d
    assert torch.equal(_ibits(unproject.unproject_camera(rows, cam, depth=dw[:, 2:2 + H * W])), _ibits(want_d))
    # no mask asked: none written (the guard of the raw call checks it)
    _raw_call(c["uv"], c["params"], c["models"], want_mask=False)


def _captured(fn):
    """fn() captured once after a warm-up on a side stream: (graph, static output)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_graph_replay_with_changed_coordinates():
    """captured once, replayed with coordinates that change an OPENCV image's iteration count.  The maxima only grow (atomicMax): without
    the call's own clear the first run's maxima would keep the image iterating, and extra trust-region steps change its bits."""
    from unidepth_amd import gtpoints, unproject
    name = "opencv_37x53_b2_iters"
    c = common.case(name)
    cam = gtpoints.prepare_camera(_camera(name), 2, "cuda")                                  # uploaded before the capture
    uv0 = c["uv"]
    centre = c["params"][:, None, 2:4]
    uv1 = (centre + np.float32(0.05) * (uv0 - centre)).astype(np.float32)                    # close to the principal point: small residuals
    info0, info1 = {}, {}
    want0 = up.unproject(uv0, c["params"], c["models"], np.float32, info0)[0]
    want1 = up.unproject(uv1, c["params"], c["models"], np.float32, info1)[0]
    assert info1["steps"][1] < info0["steps"][1] == 10
    static = torch.from_numpy(uv0).cuda()
    graph, out = _captured(lambda: unproject.unproject_camera(static, cam))
    for k, (uv, want) in enumerate(((uv1, want1), (uv0, want0), (uv1, want1))):
        static.copy_(torch.from_numpy(uv).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert common.same_bits(out.cpu().numpy(), want), f"replay {k} differs from the restatement"
        assert torch.equal(_ibits(out), _ibits(unproject.unproject_camera(torch.from_numpy(uv).cuda(), cam))), f"replay {k} differs from the eager call"


def test_graph_replay_with_swapped_camera_rows():
    from unidepth_amd import gtpoints, unproject
    name = "opencv_37x53_b2_iters"
    c = common.case(name)
    cam = gtpoints.prepare_camera(_camera(name), 2, "cuda")
    rows = cam.params.clone()
    uv = torch.from_numpy(c["uv"]).cuda()
    d = torch.from_numpy(c["depth"]).cuda()
    graph, out = _captured(lambda: unproject.unproject_camera(uv, cam, depth=d))
    for k in range(4):                                                                       # orders: swapped, original, swapped, original
        order = [1, 0] if k % 2 == 0 else [0, 1]
        cam.params.copy_(rows[order])
        graph.replay()
        torch.cuda.synchronize()
        want = up.unproject(c["uv"], c["params"][order], c["models"], np.float32, depth=c["depth"])[0]
        assert common.same_bits(out.cpu().numpy(), want), f"replay {k}"
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _gpu_case(name, "depth")[0].view(np.uint32))


@pytest.mark.parametrize("name", list(gp.CASES))
def test_round_trip_through_project_camera(name):
    """project_camera(unproject_camera(uv, cam, depth=d), cam) returns uv on the in-image regular points, within 4 x the reference's own
    round-trip error on the same inputs; EUCM points outside the mask are exempt, fewer than a tenth of any image's"""
    from unidepth_amd import reproject, unproject
    c, g = common.case(name), common.golden()
    H, W = common.shape(name)
    n_reg = up.n_regular(name)
    cam = _camera(name)
    uv = torch.from_numpy(c["uv"]).cuda()
    pts, mask = unproject.unproject_camera(uv, cam, depth=torch.from_numpy(c["depth"]).cuda(), return_mask=True)
    back = reproject.project_camera(pts, cam, image_shape=(H, W))[0].cpu().numpy()
    mask = mask.cpu().numpy()
    e = cp.uv_error(back[:, :n_reg] - c["uv"][:, :n_reg], c["uv"][:, :n_reg])
    assert np.isfinite(back[:, :n_reg]).all()
    for b, m in enumerate(c["models"]):
        keep = np.ones(n_reg, bool)
        if m == up.EUCM:
            keep = mask[b, :n_reg]
            assert (~keep).mean() < up.MASKED_SHARE, (name, b, (~keep).mean())
        bound = 4.0 * float(g["rterr." + up.MODEL_NAMES[m]])
        worst = float(e[b][keep].max())
        print(f"{name} image {b} ({up.MODEL_NAMES[m]}): round trip {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound, (name, b, up.MODEL_NAMES[m], worst, bound)
