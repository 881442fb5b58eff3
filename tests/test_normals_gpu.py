"""GPU tests of the surface normals and their metrics (unidepth_amd/normals.py -> ud_normals / ud_eval_normals, csrc/normals.hip).

normals_from_points is compared bit for bit, as integers, with the numpy fp32 restatement of tests/normals_common.py; normals_camera with
the composition gt_points + normals_from_points run on the same GPU, and with the restatement on those points; eval_normals' counts and
shares exactly and its means within 8 fp32 ulp of the restatement's float64 values.  Through the C-ABI every output sits inside a guarded
allocation (tests/layout_guard.py), masks and rgb at odd byte offsets, fp32 outputs at a 4-byte offset."""
import functools

import numpy as np
import pytest
import torch

import layout_guard as lg
import normals_common as nc

pytestmark = pytest.mark.gpu
_SENTINEL_BYTES = (0xAD, 0xDB, 0xBA, 0x7F)                     # lg.SENTINEL[torch.float32], little endian
# 8 fp32 ulp relative: the cosine has the same bits on both sides, so the only difference is acosf against float64 acos -- the 4 ulp
# OpenCL full-profile bound the device maths library is built to, one rounding for the degrees, one for the final fp32, doubled
ULP8 = 8 * 2.0 ** -23 * 1.0000001

MODEL_SETS = {
    "pinhole": (nc.PINHOLE,) * nc.B0, "eucm": (nc.EUCM,) * nc.B0, "spherical": (nc.SPHERICAL,) * nc.B0, "mei": (nc.MEI,) * nc.B0,
    "six": nc.MODELS, "iterative": (nc.OPENCV, nc.FISHEYE624, nc.OPENCV, nc.FISHEYE624, nc.PINHOLE, nc.MEI),
}


class _Out:
    """`n` elements of `dtype`, `offset` elements into a sentinel-filled allocation: the guard rows above and below are checked by
    layout_guard, the bytes of the view's own words before and after the elements here"""

    def __init__(self, n, dtype, offset=0):
        esz = torch.empty(0, dtype=dtype).element_size()
        self.words = max(1, -(-(n + offset) * esz // 4))
        self.g = lg.guarded(self.words, 1, 1, torch.float32)
        self.bytes = self.g.view.reshape(-1).view(torch.uint8)
        self.lo, self.hi = offset * esz, (offset + n) * esz
        self.t = self.bytes[self.lo:self.hi].view(dtype)

    def check(self, name, written=True):
        self.g.check_guards(name)
        want = torch.tensor(_SENTINEL_BYTES, dtype=torch.uint8, device="cuda").repeat(self.words)
        keep = torch.ones_like(want, dtype=torch.bool)
        if written:
            keep[self.lo:self.hi] = False
        assert torch.equal(self.bytes[keep], want[keep]), f"{name}: bytes beside the output were rewritten" if written else f"{name}: an absent output was written"


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _odd(t):
    """a uint8 tensor's bytes at an odd byte offset"""
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    buf[1:].copy_(t.reshape(-1).view(torch.uint8))
    return buf[1:]


def _as_np(res):
    n, v, c = res
    return dict(normals=n.cpu().numpy(), valid=v.reshape(v.shape[0], *v.shape[-2:]).cpu().numpy().astype(bool), rgb=c.cpu().numpy())


def _raw_normals(*, points=None, depth=None, cam=None, mask=None, edge_rtol=None, want=("valid", "rgb")):
    """ud_normals through the C-ABI on device tensors, every output inside a guarded allocation (absent ones too: they must stay
    untouched), the mask at an odd byte offset, twice.  -> (normals, valid bool [B,1,H,W], rgb) on the device"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    geo = points if points is not None else depth
    Bn, (H, W) = geo.shape[0], geo.shape[-2:]
    n = H * W
    bufs = dict(normals=_Out(Bn * 3 * n, torch.float32, 1), valid=_Out(Bn * n, torch.uint8, 3), rgb=_Out(Bn * 3 * n, torch.uint8, 1))
    has = {k: k == "normals" or k in want for k in bufs}
    m = None if mask is None else _odd(mask.contiguous())
    d = mk(_lib.UdNormals, points=None if points is None else points.contiguous(),
           depth=None if depth is None else depth.reshape(Bn, H, W).contiguous(), params=None if cam is None else cam.params, mask=m,
           B=Bn, H=H, W=W, mask_shared=int(mask is not None and mask.shape[0] == 1 and Bn > 1), has_rtol=int(edge_rtol is not None),
           rtol_bits=nc.f32_bits(edge_rtol or 0.0), **{k: (b.t.data_ptr() if has[k] else None) for k, b in bufs.items()})
    if cam is not None:
        for b in range(Bn):
            d.model[b] = cam.models[b]
    runs = []
    for _ in range(2):
        check(_lib.lib.ud_normals(d, cur_stream()), "ud_normals")
        torch.cuda.synchronize()
        runs.append({k: b.t.clone() for k, b in bufs.items() if has[k]})
    for k, b in bufs.items():
        b.check(k, has[k])
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    r = runs[0]
    if "valid" in r:
        assert int(r["valid"].max()) <= 1
    return (r["normals"].view(Bn, 3, H, W), r["valid"].view(Bn, 1, H, W).bool() if "valid" in r else None,
            r["rgb"].view(Bn, 3, H, W) if "rgb" in r else None)


def _cam(models):
    return nc.wc.prepared(nc.rows(models), models)


def _composition(depth, cam, mask, edge_rtol):
    """what normals_camera must equal: gt_points, then normals_from_points with mask & (depth > 0) and the depth.  -> (result, points)"""
    from unidepth_amd import gtpoints, normals
    pts = gtpoints.gt_points(depth, cam)
    pos = depth.reshape(depth.shape[0], 1, *depth.shape[-2:]) > 0
    eff = pos if mask is None else pos & mask.reshape(-1, 1, *depth.shape[-2:]).bool()
    return normals.normals_from_points(pts, mask=eff, depth=depth, edge_rtol=edge_rtol, return_mask=True, return_rgb=True), pts


def _check_depth_form(depth, mask, models, edge_rtol, what, raw=True, conditions=False):
    """normals_camera (the Python surface, and the C-ABI with guards for closed-form batches) == the composition == the restatement on
    the composition's points; returns the restatement's result"""
    from unidepth_amd import normals
    cam = _cam(models)
    d, m = _dev(depth), None if mask is None else _dev(mask)
    comp, pts = _composition(d, cam, m, edge_rtol)
    want = _as_np(comp)
    got = _as_np(normals.normals_camera(d, cam, mask=m, edge_rtol=edge_rtol, return_mask=True, return_rgb=True))
    nc.assert_same(got, want, f"{what}: normals_camera vs the composition")
    if raw and not any(k in (nc.OPENCV, nc.FISHEYE624) for k in models):
        nc.assert_same(_as_np(_raw_normals(depth=d, cam=cam, mask=m, edge_rtol=edge_rtol)), want, f"{what}: ud_normals (depth form) vs the composition")
    dn = np.asarray(depth).reshape(depth.shape[0], *depth.shape[-2:])
    eff = dn > 0 if mask is None else (dn > 0) & (np.broadcast_to(np.asarray(mask).reshape(-1, *dn.shape[-2:]), dn.shape) != 0)
    r = nc.restate_normals(pts.cpu().numpy(), eff, dn, edge_rtol)
    nc.assert_same(got, r, f"{what}: normals_camera vs the restatement")
    if conditions:
        nc.check_conditions(r, edge_rtol is not None)
    return r


# ---- the points form -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", (None, nc.EDGE_RTOL), ids=("no_edge", "edge"))
def test_points_form_against_the_restatement(edge):
    """the scene's points through the six models (gt_points, downloaded for the restatement): normals, valid and rgb bit for bit, through
    the C-ABI with guards and through the Python surface, with and without a separate depth; the scene's conditions asserted"""
    from unidepth_amd import gtpoints, normals
    depth, mask = nc.scene()
    d, m = _dev(depth), _dev(mask)
    pts = gtpoints.gt_points(d, _cam(nc.MODELS))
    pn = pts.cpu().numpy()
    for use_depth in (True, False):
        r = nc.restate_normals(pn, mask, depth if use_depth else None, edge)
        nc.check_conditions(r, edge is not None)
        kw = dict(mask=m, depth=d if use_depth else None, edge_rtol=edge)
        nc.assert_same(_as_np(_raw_normals(points=pts, **kw)), r, f"ud_normals, depth={use_depth}")
        nc.assert_same(_as_np(normals.normals_from_points(pts, return_mask=True, return_rgb=True, **kw)), r, f"normals_from_points, depth={use_depth}")
    only = normals.normals_from_points(pts, mask=m.bool()[:, 0], depth=d[:, 0].double(), edge_rtol=edge)      # other dtypes and shapes, one output
    r = nc.restate_normals(pn, mask, depth, edge)
    assert isinstance(only, torch.Tensor) and nc.same_bits(only.cpu().numpy(), r["normals"])
    n, _, _ = _raw_normals(points=pts, mask=m, depth=d, edge_rtol=edge, want=())                               # absent outputs stay untouched
    assert nc.same_bits(n.cpu().numpy(), r["normals"])


def test_known_answers():
    from unidepth_amd import normals

    def run(pts):
        n, v = normals.normals_from_points(_dev(pts), return_mask=True)
        return n.cpu().numpy(), v.cpu().numpy()
    nc.check_known_answer(run)


# ---- the depth form ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MODEL_SETS))
@pytest.mark.parametrize("edge", (None, nc.EDGE_RTOL), ids=("no_edge", "edge"))
def test_depth_form_against_the_composition(name, edge):
    """each closed-form model alone, the six-model batch and a batch of OPENCV / Fisheye624 members: every output of normals_camera has
    the bits of gt_points + normals_from_points on the same GPU, and of the restatement on those points"""
    depth, mask = nc.scene()
    _check_depth_form(depth, mask, MODEL_SETS[name], edge, name, conditions=True)


@pytest.mark.parametrize("size", ((2, 2), (3, 3), (1, 7), (5, 1), (7, 31), (8, 32), (9, 33), (8, 31), (7, 33), (12, 63), (12, 64), (12, 65),
                                  (3, 85), (15, 17), (16, 16), (1, 257), (257, 1), (9, 130)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_where_a_tiled_stencil_can_go_wrong(size):
    """2 x 2 (every pixel one-sided both ways), 3 x 3, 1 x 7 and 5 x 1 (no valid pixel, all-zero output), the 32 x 8 tile's width and
    height -1, +0, +1, widths 63 / 64 / 65, pixel counts 255 / 256 / 257: both forms, the six models, without and with the edge test
    (which drops every vertical neighbour of the scene at a height below about 8: its depth grows by 0.9 / H per row)"""
    from unidepth_amd import normals
    H, W = size
    depth, mask = nc.scene(H, W)
    if size == (2, 2):                                  # nothing masked: all four pixels valid, each from two one-sided differences
        depth, mask = np.array(depth), np.ones_like(mask)
        depth[:] = np.array([[2.0, 2.1], [2.2, 2.35]], np.float32)
    r = _check_depth_form(depth, mask, nc.MODELS, None, f"{H}x{W}")
    _check_depth_form(depth, mask, nc.MODELS, nc.EDGE_RTOL, f"{H}x{W}, edge")
    if min(H, W) == 1:
        n, v, c = normals.normals_camera(_dev(depth), _cam(nc.MODELS), mask=_dev(mask), return_mask=True, return_rgb=True)
        assert not bool(n.any()) and not bool(v.any()) and not bool(c.any()) and not r["valid"].any()
    elif size == (2, 2):
        assert r["valid"].all() and r["one_sided"].all()
    else:
        assert r["valid"].mean() > 0.7


def test_one_image_and_a_shared_mask():
    """B = 1, and B = 3 with one mask for all images ([1,1,H,W], mask_shared): both forms"""
    from unidepth_amd import normals
    depth, mask = nc.scene()
    _check_depth_form(depth[:1], mask[:1], (nc.EUCM,), nc.EDGE_RTOL, "B = 1")
    models = (nc.MEI, nc.PINHOLE, nc.SPHERICAL)
    r = _check_depth_form(depth[:3], mask[:1], models, nc.EDGE_RTOL, "shared mask")
    assert 0.5 < r["valid"].mean() < 0.95
    pts = _composition(_dev(depth[:3]), _cam(models), None, None)[1]
    rp = nc.restate_normals(pts.cpu().numpy(), mask[:1], None, nc.EDGE_RTOL)
    nc.assert_same(_as_np(_raw_normals(points=pts, mask=_dev(mask[:1]), edge_rtol=nc.EDGE_RTOL)), rp, "points form, shared mask")
    nc.assert_same(_as_np(normals.normals_from_points(pts, mask=_dev(mask[:1]), edge_rtol=nc.EDGE_RTOL, return_mask=True, return_rgb=True)), rp,
                   "normals_from_points, shared mask")


def test_special_values():
    """depth 0, -0.0, negative, NaN, +-inf and 1e-30 at the head of the first rows (depth form, six models); points of 1e30 (the cross
    product overflows), neighbours 1e-30 apart (m underflows to 0), coincident neighbours, non-finite coordinates; and mirrored clouds,
    where every valid normal has n . P <= 0 and the flip branch is taken on at least half of them"""
    depth, mask = nc.special_depth(), nc.scene()[1]
    for edge in (None, nc.EDGE_RTOL):
        r = _check_depth_form(depth, mask, nc.MODELS, edge, "special depth")
        assert not r["valid"][:, 0, 0:3].any() and not r["valid"][:, 1, 1:3].any() and r["valid"].mean() > 0.5
    r = _check_depth_form(depth, mask, MODEL_SETS["iterative"], None, "special depth, iterative")
    pts = nc.special_points()
    r = nc.restate_normals(pts)
    got = _as_np(_raw_normals(points=_dev(pts)))
    nc.assert_same(got, r, "special points")
    nc.assert_same(_as_np(_raw_normals(points=_dev(pts), edge_rtol=0.5)), nc.restate_normals(pts, None, None, 0.5), "special points, edge")
    assert not got["valid"][0].any() and not got["valid"][1].any() and not got["normals"][:2].any()
    assert not got["valid"][2, 3, 4:6].any() and not got["valid"][2, 6, 2] and not got["valid"][2, 6, 6] and not got["valid"][2, 7, 8]
    for b in (3, 4):
        assert got["valid"][b].all()
        assert ((got["normals"][b].astype(np.float64) * pts[b]).sum(axis=0) <= 0).all()
        assert r["flipped"][b].sum() >= 0.5 * r["valid"][b].sum()


def test_graph_replay_after_inputs_were_rewritten():
    """captured once with a PreparedCamera; replayed after the depth, the mask and the camera's parameter rows were rewritten in place:
    each replay equals a fresh call and the composition"""
    from unidepth_amd import gtpoints, normals
    depth0, mask0 = nc.scene()
    other = nc.pred_depth()
    models = (nc.MEI, nc.SPHERICAL, nc.EUCM, nc.PINHOLE, nc.EUCM, nc.SPHERICAL)
    base = _cam(models)
    depth, mask = _dev(depth0), _dev(mask0)
    cam = gtpoints.PreparedCamera(base.params.clone(), base.models)
    fn = lambda: normals.normals_camera(depth, cam, mask=mask, edge_rtol=nc.EDGE_RTOL, return_mask=True, return_rgb=True)       # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    for k in range(3):
        depth.copy_(_dev(other) if k % 2 == 0 else torch.flip(depth, (0, 3)))
        mask.copy_(torch.flip(mask, (2,)) if k % 2 == 0 else torch.flip(mask, (0,)))
        cam.params[:, :2].mul_(1.03 if k % 2 == 0 else 0.95)
        graph.replay()
        torch.cuda.synchronize()
        got = _as_np(static)
        nc.assert_same(got, _as_np(fn()), f"replay {k} vs eager")
        nc.assert_same(got, _as_np(_composition(depth, cam, mask, nc.EDGE_RTOL)[0]), f"replay {k} vs the composition")
        assert 0.5 < got["valid"].mean() < 0.95


# ---- the metrics -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _metric_inputs():
    """gt = the scene's normals, pred = the normals of the same scene with another noise seed, six models, on the device (never written)"""
    from unidepth_amd import normals
    depth, mask = nc.scene()
    cam = _cam(nc.MODELS)
    return normals.normals_camera(_dev(depth), cam, mask=_dev(mask)), normals.normals_camera(_dev(nc.pred_depth()), cam, mask=_dev(mask)), _dev(mask)


def _raw_eval(gt, pred, mask, thresholds, want_error=True):
    """ud_eval_normals through the C-ABI: guarded outputs, the mask at an odd byte offset, a dirty workspace, twice (the second call on
    the workspace the first one left).  -> (out [3 + T, B], count [B], error [B,H,W] or None)"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    Bn, _, H, W = gt.shape
    T = len(thresholds)
    bufs = dict(out=_Out((3 + T) * Bn, torch.float32, 1), count=_Out(Bn, torch.int64, 1), error=_Out(Bn * H * W, torch.float32, 1))
    has = dict(out=True, count=True, error=want_error)
    nbytes = int(_lib.lib.ud_eval_normals_work_bytes(Bn, H, W, T))
    work = torch.randint(0, 256, (nbytes + 16,), dtype=torch.uint8, device="cuda")
    work = work[(-work.data_ptr()) % 16:][:nbytes]
    m = None if mask is None else _odd(mask.contiguous())
    d = mk(_lib.UdEvalNormals, gt=gt.contiguous(), pred=pred.contiguous(), mask=m, B=Bn, H=H, W=W, T=T,
           mask_shared=int(mask is not None and mask.shape[0] == 1 and Bn > 1), **{k: (b.t.data_ptr() if has[k] else None) for k, b in bufs.items()})
    for k, t in enumerate(thresholds):
        d.cos_bits[k] = nc.f32_bits(float(nc.cos_of(t)))
    runs = []
    for _ in range(2):
        check(_lib.lib.ud_eval_normals(d, work.data_ptr(), nbytes, cur_stream()), "ud_eval_normals")
        torch.cuda.synchronize()
        runs.append({k: b.t.clone() for k, b in bufs.items() if has[k]})
    for k, b in bufs.items():
        b.check(k, has[k])
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    r = runs[0]
    return r["out"].view(3 + T, Bn), r["count"], r["error"].view(Bn, H, W) if want_error else None


def _check_eval(res, want, thresholds, what):
    """counts and shares exactly; mean, median, rmse and the error map within 8 fp32 ulp of the restatement; returns the worst ratio"""
    assert res["count"].dtype == torch.int64 and res["count"].cpu().tolist() == want["count"].tolist(), what
    worst = 0.0
    for t in thresholds:
        a = res[f"a_{t}"].cpu().numpy()
        assert a.dtype == np.float32 and nc.same_bits(a, want[f"a_{t}"].astype(np.float32)), (what, t, a, want[f"a_{t}"])
    for k in ("mean", "median", "rmse"):
        got, ref = res[k].cpu().numpy().astype(np.float64), want[k]
        assert (np.isnan(got) == np.isnan(ref)).all(), (what, k, got, ref)
        ok = ~np.isnan(ref)
        ratio = np.abs(got[ok] - ref[ok]) / (ULP8 * np.abs(ref[ok]) + 1e-300)
        ratio = np.where(got[ok] == ref[ok], 0.0, ratio)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (ratio <= 1.0).all(), (what, k, got, ref, ratio)
    if "error" in res:
        got, ref = res["error"].cpu().numpy().astype(np.float64).reshape(want["error"].shape), want["error"]
        assert (np.isnan(got) == np.isnan(ref)).all(), what
        ok = ~np.isnan(ref)
        ratio = np.where(got[ok] == ref[ok], 0.0, np.abs(got[ok] - ref[ok]) / (ULP8 * np.abs(ref[ok]) + 1e-300))
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (ratio <= 1.0).all(), (what, "error", float(ratio.max()))
    return worst


def _res_of_raw(out, count, err, thresholds):
    res = {"mean": out[0], "median": out[1], "rmse": out[2], "count": count}
    for k, t in enumerate(thresholds):
        res[f"a_{t}"] = out[3 + k]
    if err is not None:
        res["error"] = err
    return res


def test_eval_normals_against_the_restatement():
    """the scene against the same scene with another noise seed (every share of every image inside (0.05, 0.95): asserted on the
    restatement alone), the Python surface and the C-ABI with guards and a dirty workspace"""
    from unidepth_amd import normals
    gt, pred, mask = _metric_inputs()
    want = nc.restate_eval(gt.cpu().numpy(), pred.cpu().numpy(), mask.cpu().numpy())
    for t in nc.THRESHOLDS:
        assert (want[f"a_{t}"] > 0.05).all() and (want[f"a_{t}"] < 0.95).all(), (t, want[f"a_{t}"])
    res = normals.eval_normals(gt, pred, mask, return_error=True)
    assert list(res) == ["mean", "median", "rmse", "a_11.25", "a_22.5", "a_30.0", "count", "error"] and res["error"].shape == (nc.B0, 1, nc.H0, nc.W0)
    worst = _check_eval(res, want, nc.THRESHOLDS, "eval_normals")
    raw = _res_of_raw(*_raw_eval(gt, pred, mask, nc.THRESHOLDS), nc.THRESHOLDS)
    worst = max(worst, _check_eval(raw, want, nc.THRESHOLDS, "ud_eval_normals"))
    for k in ("mean", "median", "rmse"):
        assert torch.equal(raw[k].view(torch.int32), res[k].view(torch.int32)), k                              # two calls, the same bits
    print(f"eval_normals: worst |got - restatement| / (8 ulp) = {worst:.3f}")
    plain = normals.eval_normals(gt, pred, mask.bool()[:, 0])
    assert "error" not in plain and torch.equal(plain["mean"].view(torch.int32), res["mean"].view(torch.int32))
    raw = _res_of_raw(*_raw_eval(gt, pred, mask, nc.THRESHOLDS, want_error=False), nc.THRESHOLDS)              # the absent map stays untouched
    _check_eval(raw, want, nc.THRESHOLDS, "ud_eval_normals without the error map")


def test_eval_normals_special_cases():
    """an image without a usable pixel (NaN rows, count 0), identical inputs, opposite inputs (180), n = 1 and n = 2 (the lower median),
    vectors that are not unit vectors, zero and non-finite vectors dropped, a shared mask, T = 1 and T = 8"""
    from unidepth_amd import normals
    g = np.random.RandomState(9601)
    H, W = 5, 7
    gt = g.normal(size=(7, 3, H, W)).astype(np.float32)
    pred = g.normal(size=(7, 3, H, W)).astype(np.float32)
    mask = np.ones((7, 1, H, W), np.uint8)
    mask[0] = 0                                         # no usable pixel
    pred[1] = gt[1]                                     # identical
    gt[2] = np.array([0.0, 0.0, -2.0], np.float32)[:, None, None]          # exact lengths: the cosine is exactly -1
    pred[2] = -gt[2]                                    # opposite
    mask[3] = 0
    mask[3, 0, 2, 3] = 1                                # n = 1
    mask[4] = 0
    mask[4, 0, 1, 1] = mask[4, 0, 3, 5] = 1             # n = 2
    gt[5] *= 7.5                                        # lengths other than 1
    gt[6, :, 0, 0], gt[6, 0, 0, 1], pred[6, 1, 0, 2], pred[6, :, 0, 3] = 0.0, np.nan, np.inf, 0.0
    gt[6, :, 1, 0], pred[6, :, 1, 0] = 1e30, 1e30       # the squares overflow: dropped
    for thr in (nc.THRESHOLDS, (45.0,), (5.0, 11.25, 22.5, 30.0, 60.0, 90.0, 120.0, 180.0)):
        want = nc.restate_eval(gt, pred, mask, thr)
        res = normals.eval_normals(_dev(gt), _dev(pred), _dev(mask), thresholds=thr, return_error=True)
        _check_eval(res, want, thr, f"T = {len(thr)}")
        _check_eval(_res_of_raw(*_raw_eval(_dev(gt), _dev(pred), _dev(mask), thr), thr), want, thr, f"raw, T = {len(thr)}")
        assert want["count"].tolist() == [0, 35, 35, 1, 2, 35, 30]
        assert all(bool(torch.isnan(res[k][0])) for k in res if k not in ("count", "error"))
        assert float(res["mean"][2]) == 180.0 and float(res["median"][2]) == 180.0 and float(res["rmse"][2]) == 180.0
        assert float(res["median"][1]) < 0.05 and float(res[f"a_{thr[0]}"][1]) == 1.0 and float(res[f"a_{thr[0]}"][2]) == 0.0
        e4 = want["error"][4][mask[4, 0] != 0]
        assert float(res["median"][4]) == pytest.approx(e4.min(), rel=1e-6) and float(res["median"][3]) == pytest.approx(float(res["mean"][3]), rel=1e-6)
    shared = np.ones((1, 1, H, W), np.uint8)
    shared[0, 0, ::2, 1::2] = 0
    _check_eval(normals.eval_normals(_dev(gt), _dev(pred), _dev(shared)), nc.restate_eval(gt, pred, shared), nc.THRESHOLDS, "shared mask")
    _check_eval(normals.eval_normals(_dev(gt), _dev(pred)), nc.restate_eval(gt, pred), nc.THRESHOLDS, "no mask")


@pytest.mark.parametrize("size", ((1, 4095), (64, 64), (1, 4097), (3, 2731)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_eval_normals_around_the_chunk_size(size):
    """pixel counts 4095 / 4096 / 4097 (one chunk of 4096 pixels, and one pixel into the second) and 8193 (three chunks)"""
    from unidepth_amd import normals
    H, W = size
    g = np.random.RandomState(9700 + W)
    gt = g.normal(size=(2, 3, H, W)).astype(np.float32)
    pred = (gt + 0.5 * g.normal(size=gt.shape)).astype(np.float32)
    mask = (g.uniform(size=(2, 1, H, W)) > 0.2).astype(np.uint8)
    mask[..., -1] = 1                                   # the last pixel counts
    want = nc.restate_eval(gt, pred, mask)
    _check_eval(normals.eval_normals(_dev(gt), _dev(pred), _dev(mask), return_error=True), want, nc.THRESHOLDS, f"{H}x{W}")
    _check_eval(_res_of_raw(*_raw_eval(_dev(gt), _dev(pred), _dev(mask), nc.THRESHOLDS), nc.THRESHOLDS), want, nc.THRESHOLDS, f"raw {H}x{W}")


def test_eval_normals_graph_replay():
    """captured once; replayed after the prediction and the mask were rewritten in place: each replay has the bits of a fresh call"""
    from unidepth_amd import normals
    gt, pred0, mask0 = _metric_inputs()
    pred, mask = pred0.clone(), mask0.clone()
    fn = lambda: normals.eval_normals(gt, pred, mask, return_error=True)       # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    for k in range(3):
        pred.copy_(torch.flip(pred0, (0,)) if k % 2 == 0 else gt)
        mask.copy_(torch.flip(mask0, (3,)) if k % 2 == 0 else mask0)
        graph.replay()
        torch.cuda.synchronize()
        fresh = fn()
        for key in static:
            a, b = static[key], fresh[key]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), (k, key)
        _check_eval(static, nc.restate_eval(gt.cpu().numpy(), pred.cpu().numpy(), mask.cpu().numpy()), nc.THRESHOLDS, f"replay {k}")
        assert int(static["count"].min()) > 1000
