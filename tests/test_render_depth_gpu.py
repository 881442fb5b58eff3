"""GPU tests of the splatting side (csrc/splat.hip through ud_splat / ud_depth_minpool and unidepth_amd/reproject.py) against the numpy
restatement of tools/make_golden_render_depth.py (pinned to the reference's own arrays by tests/test_render_depth_cpu.py).

The kernel tests call the C-ABI with every output inside a tests/layout_guard.py guard allocation, on a work buffer pre-filled with
0xA5, twice: the guard bands and the outputs that were not requested must keep their bits, and both calls must give the same bits.
Nearest mode is bit-exact in depth, index, rgb and count.  Mean mode is exact in count, and its depth is within
2^-25 + (2^-24 + 2^-50) |m| of the float64 mean m: every point is rounded to a multiple of 2^-24 (half a step, 2^-25, which the mean
keeps), the int64 sum is exact, the double quotient is off by 2^-53 relative twice (2^-50 covers it) and the store rounds once to fp32.
Shapes follow the kernel's constants: CHUNK = 1024 points per workgroup of the splat pass, RTILE = 256 pixels per workgroup of resolve."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(ROOT, "tests", "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)
_spec = importlib.util.spec_from_file_location("make_golden_render_depth", os.path.join(ROOT, "tools", "make_golden_render_depth.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

CHUNK, RTILE = 1024, 256


def _guard(n, dtype):
    """`n` elements of `dtype` inside a guard allocation, seen as a flat tensor."""
    words = max(1, -(-n * torch.empty(0, dtype=dtype).element_size() // 4))
    g = lg.guarded(words, 1, 1, torch.float32)
    return g, g.view.reshape(-1).view(dtype)[:n]


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def _mean_bound(m):
    return 2.0 ** -25 + (2.0 ** -24 + 2.0 ** -50) * np.abs(m)


def _call(xyz, strides, n_points, B, hw, K, T=None, offsets=None, color=None, mode="nearest", pixel_offset=0.0, rounding="floor",
          depth_range=None, want_index=True, want_count=True):
    """ud_splat on guarded outputs and a 0xA5 work buffer, twice; returns the host outputs (None where not requested)."""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    H, W = hw
    nearest = mode == "nearest"
    want_index = want_index and nearest
    dev = {k: (None if v is None else torch.as_tensor(v).contiguous().cuda()) for k, v in dict(xyz=xyz, K=K, T=T, offsets=offsets, color=color).items()}
    f32_color = color is not None and dev["color"].dtype == torch.float32
    px = B * H * W
    gd, depth = _guard(px, torch.float32)
    gi, index = _guard(px, torch.int32)
    gn, count = _guard(px, torch.int32)
    gc, rgb = _guard(3 * px, torch.float32 if f32_color else torch.uint8)
    before = [_bits(t) for t in (depth, index, count, rgb)]
    nbytes = int(_lib.lib.ud_splat_work_bytes(B, H, W))
    assert nbytes == 12 * px
    work = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    flags = (_lib.UD_SPLAT_TRUNC if rounding == "trunc" else 0) | (_lib.UD_SPLAT_RANGE if depth_range is not None else 0)
    d = mk(_lib.UdSplat, depth=depth.data_ptr(), index=index.data_ptr() if want_index else None, count=count.data_ptr() if want_count else None,
           rgb=rgb.data_ptr() if color is not None else None, work=work, work_bytes=nbytes, batch_stride=strides[0], point_stride=strides[1],
           comp_stride=strides[2], n_points=n_points, B=B, H=H, W=W, nK=dev["K"].reshape(-1, 3, 3).shape[0],
           nT=0 if T is None else dev["T"].reshape(-1, 3, 4).shape[0], mode=_lib.UD_SPLAT_NEAREST if nearest else _lib.UD_SPLAT_MEAN, flags=flags,
           color_f32=int(f32_color), pixel_offset=pixel_offset, dmin=0.0 if depth_range is None else depth_range[0],
           dmax=0.0 if depth_range is None else depth_range[1], **{k: v for k, v in dev.items() if v is not None})
    check(_lib.lib.ud_splat(d, cur_stream()), "ud_splat")
    torch.cuda.synchronize()
    first = [_bits(t) for t in (depth, index, count, rgb)]
    check(_lib.lib.ud_splat(d, cur_stream()), "ud_splat")          # the work buffer now holds the first call's words
    torch.cuda.synchronize()
    second = [_bits(t) for t in (depth, index, count, rgb)]
    for g in (gd, gi, gn, gc):
        g.check_guards()
    for a, b in zip(first, second):
        assert np.array_equal(a, b), "two calls gave different bits"
    for asked, a, b in zip((True, want_index, want_count, color is not None), before, second):
        assert asked or np.array_equal(a, b), "an output that was not requested was written"
    return {"depth": depth.cpu().numpy().reshape(B, H, W),
            "index": index.cpu().numpy().reshape(B, H, W) if want_index else None,
            "count": count.cpu().numpy().reshape(B, H, W) if want_count else None,
            "rgb": rgb.cpu().numpy().reshape(B, 3, H, W) if color is not None else None}


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
        assert np.array_equal(np.isnan(out["depth"]), np.isnan(m))
        ok = ~np.isnan(m)
        err = np.abs(out["depth"].astype(np.float64) - m)[ok]
        print(f"mean mode: worst error / bound {float((err / _mean_bound(m[ok])).max()) if err.size else 0.0:.3f}")
        assert (err <= _mean_bound(m[ok])).all()
        assert (out["depth"][ref["count"] == 0] == 0).all()


def _splat(clouds, K, hw, layout="rows", colors=None, T=None, mode="nearest", **kw):
    """ud_splat on a list of per-image clouds [n,3] laid out as [B,N,3] rows, [B,3,N] planes or packed rows + offsets, checked against
    restate(); returns (outputs, restatement)."""
    B = len(clouds)
    ref = mg.restate(clouds, K, hw, T=T, mode=mode, colors=colors if mode == "nearest" else None,
                     **{k: v for k, v in kw.items() if k in ("pixel_offset", "rounding", "depth_range")})
    if mode != "nearest":
        colors = None
    offsets = None
    if layout == "packed":
        n = sum(c.shape[0] for c in clouds)
        pad = np.tile(np.array([[0.0, 0.0, 0.5]], dtype=np.float32), (5, 1))       # rows behind offsets[B]: owned by no image, never splatted
        xyz = np.concatenate(list(clouds) + [pad])
        color = None if colors is None else np.concatenate(list(colors) + [np.full((5, 3), 77, dtype=colors[0].dtype)])
        offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
        strides, n_points = (0, 3, 1), n + 5
    else:
        n = clouds[0].shape[0]
        assert all(c.shape[0] == n for c in clouds)
        xyz = np.stack(clouds)
        color = None if colors is None else np.stack(colors)
        strides, n_points = (3 * n, 3, 1), n
        if layout == "planar":
            xyz = np.ascontiguousarray(xyz.transpose(0, 2, 1))
            color = None if color is None else np.ascontiguousarray(color.transpose(0, 2, 1))
            strides = (3 * n, 1, n)
    out = _call(xyz, strides, n_points, B, hw, K, T=T, offsets=offsets, color=color, mode=mode, **kw)
    _compare(out, ref, mode)
    return out, ref


ZS = np.array([0.75, 1.0, 1.5, 2.0, 3.25], dtype=np.float64)           # few depths: ties on a pixel are common, the index decides them


def _scene(B, N, hw, seed, per_image=True, f32_colors=False):
    """clouds aimed at [-1.5, W + 1.5) x [-1.5, H + 1.5) with a few z <= 0 / NaN / inf points, K (skewed) and T per image or shared"""
    H, W = hw
    g = np.random.default_rng(seed)
    nm = B if per_image else 1
    f = 0.8 * max(W, H) + 1.3
    K = np.zeros((nm, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 1], K[:, 2, 2] = f + np.arange(nm), f - 0.7 + np.arange(nm), 0.05, 1.0
    K[:, 0, 2], K[:, 1, 2] = W / 2 + 0.3, H / 2 - 0.2
    ang = 0.02 * (1 + np.arange(nm))
    T = np.zeros((nm, 3, 4))
    T[:, 0, 0], T[:, 0, 2], T[:, 2, 0], T[:, 2, 2], T[:, 1, 1] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang), 1.0
    T[:, :, 3] = np.array([0.01, -0.02, 0.1]) * (1 + np.arange(nm))[:, None]
    clouds, colors = [], []
    for b in range(B):
        u, v = g.uniform(-1.5, W + 1.5, N), g.uniform(-1.5, H + 1.5, N)
        z = g.choice(ZS, N)
        k = K[b if per_image else 0]
        y = (v - k[1, 2]) * z / k[1, 1]
        x = ((u - k[0, 2]) * z - k[0, 1] * y) / k[0, 0]
        p = np.stack([x, y, z], axis=-1).astype(np.float32)
        if N >= 16:
            i = g.choice(N, 8, replace=False)
            p[i[0], 2], p[i[1], 2], p[i[2], 2], p[i[3], 2], p[i[4], 0], p[i[5], 1] = -1.0, 0.0, np.nan, np.inf, np.nan, -np.inf
        clouds.append(p)
        colors.append(g.random((N, 3), dtype=np.float32) if f32_colors else g.integers(0, 256, (N, 3), dtype=np.uint8))
    return clouds, colors, K.astype(np.float32), T.astype(np.float32)


def _resplit(clouds, colors, sizes):
    """the same rows dealt to images of the given sizes (the packed layout takes clouds of different lengths)"""
    allp, allc = np.concatenate(clouds), np.concatenate(colors)
    assert sum(sizes) == allp.shape[0]
    cuts = np.cumsum([0] + list(sizes))
    return [allp[a:b] for a, b in zip(cuts[:-1], cuts[1:])], [allc[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


SHAPES = [(1, 1, (1, 1)), (1, CHUNK - 1, (7, 9)), (1, CHUNK, (7, 9)), (3, CHUNK + 1, (7, 9)), (3, 3 * CHUNK + 17, (3, RTILE + 44)), (1, 2 * CHUNK, (1, 1))]


@pytest.mark.parametrize("mode", ["nearest", "mean"])
@pytest.mark.parametrize("layout", ["rows", "planar", "packed"])
@pytest.mark.parametrize("B,N,hw", SHAPES)
def test_shapes_by_kernel_constants(B, N, hw, layout, mode):
    """N = 1, CHUNK - 1, CHUNK, CHUNK + 1 and a few chunks; destinations 1 x 1, 7 x 9 and one wider than a resolve tile; B = 1 and 3 with
    per-image K and T; rows, planes and packed rows"""
    clouds, colors, K, T = _scene(B, N, hw, seed=N * 10 + B)
    if layout == "packed" and B == 3:
        clouds, colors = _resplit(clouds, colors, (N + 7, 2 * N - 30, 23))
    out, ref = _splat(clouds, K, hw, layout=layout, colors=colors, T=T, mode=mode)
    if N >= CHUNK - 1:
        assert ref["count"].max() >= 2 and ref["count"].sum() < B * N            # pixels with several points, and points that were dropped


@pytest.mark.parametrize("mode", ["nearest", "mean"])
@pytest.mark.parametrize("layout", ["rows", "packed"])
def test_shared_intrinsics_and_transform(layout, mode):
    clouds, colors, K, T = _scene(3, CHUNK + 1, (7, 9), seed=5, per_image=False)
    assert K.shape[0] == 1 and T.shape[0] == 1
    _splat(clouds, K, (7, 9), layout=layout, colors=colors, T=T, mode=mode)
    _splat(clouds, K, (7, 9), layout=layout, colors=colors, mode=mode)               # and without a transform


@pytest.mark.parametrize("layout", ["rows", "planar", "packed"])
def test_every_point_on_one_pixel(layout):
    """N = 5000 points inside one cell of a 3 x 5 image: the smallest z wins, among equal z the smallest index; the count is N"""
    N, hw = 5000, (3, 5)
    g = np.random.default_rng(7)
    z = g.choice(ZS, N)
    z[:40] = 3.25                                                                    # the first minimum is not at the front
    p = np.stack([(3.25 + 0.5 * g.random(N)) * z, (1.25 + 0.5 * g.random(N)) * z, z], axis=-1).astype(np.float32)
    colors = [g.integers(0, 256, (N, 3), dtype=np.uint8)]
    out, ref = _splat([p], np.eye(3, dtype=np.float32)[None], hw, layout=layout, colors=colors)
    first = int(np.nonzero(p[:, 2] == np.float32(0.75))[0][0])
    assert first >= 40 and (p[:, 2] == np.float32(0.75)).sum() > 100
    assert out["count"][0, 1, 3] == N and out["count"].sum() == N and out["index"][0, 1, 3] == first and out["depth"][0, 1, 3] == np.float32(0.75)
    assert out["rgb"][0, :, 1, 3].tolist() == colors[0][first].tolist() and (out["index"].reshape(-1) >= 0).sum() == 1
    out, ref = _splat([p], np.eye(3, dtype=np.float32)[None], hw, layout=layout, mode="mean")
    assert out["count"][0, 1, 3] == N


EDGE_W = 8


def _edge_points():
    """u = x exactly (K = identity, z = 1): u = 0, -0.0, -0.5, W - 2^-k, W, and the same in v"""
    us = [0.0, -0.0, -0.5, -1.0, EDGE_W - 2.0 ** -20, EDGE_W - 2.0 ** -10, EDGE_W - 0.5, float(EDGE_W), 3.0, 2.9999998]
    rows = [[u, 0.5, 1.0] for u in us] + [[0.5, 0.0, 1.0], [0.5, -0.0, 1.0], [0.5, -0.5, 1.0], [0.5, 2.0 - 2.0 ** -22, 1.0], [0.5, 2.0, 1.0]]
    return np.array(rows, dtype=np.float32)


@pytest.mark.parametrize("mode", ["nearest", "mean"])
def test_cell_edges_under_floor_trunc_and_offset(mode):
    p, K, hw = _edge_points(), np.eye(3, dtype=np.float32)[None], (2, EDGE_W)
    f, _ = _splat([p], K, hw, mode=mode)
    # floor: 0 and -0.0 stay in column 0, -0.5 and -1 leave; W - 2^-k stays in column W - 1, W leaves; rows likewise
    assert f["count"][0, 0].tolist() == [2 + 2, 0, 1, 1, 0, 0, 0, 3] and f["count"][0, 1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    t, _ = _splat([p], K, hw, mode=mode, rounding="trunc")
    assert t["count"][0, 0].tolist() == [3 + 3, 0, 1, 1, 0, 0, 0, 3] and t["count"][0, 1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    o, _ = _splat([p], K, hw, mode=mode, pixel_offset=0.5)
    # + 0.5: u = -0.5 enters column 0, u = -1 and u >= W - 0.5 leave; v = 0.5 moves to row 1; the points at u = 0.5 move to column 1, those
    # with v in {0, -0.0, -0.5} into row 0, v >= 1.5 leaves
    assert o["count"][0, 1].tolist() == [3, 0, 0, 2, 0, 0, 0, 0] and o["count"][0, 0].tolist() == [0, 3, 0, 0, 0, 0, 0, 0]
    _splat([p], K, hw, mode=mode, pixel_offset=0.5, rounding="trunc")


@pytest.mark.parametrize("mode", ["nearest", "mean"])
def test_invalid_points_and_range_ends(mode):
    """z <= 0, NaN, inf and w = 0 points; depth_range ends met exactly and one ulp outside"""
    K = np.array([[[2.0, 0, 0], [0, 2.0, 0], [0, 0, 1.0]]], dtype=np.float32)
    P = lambda u, z: [u * z / 2.0, 0.25 * z, z]                                      # noqa: E731
    one = np.float32(1.0)
    lo, hi = np.float32(1.25), np.float32(2.5)
    zs = [3.0, -1.0, 0.0, np.nan, np.inf, -np.inf, lo, hi, np.nextafter(lo, -one), np.nextafter(hi, np.float32(9.0)), 2.0, -0.0]
    p = np.array([P(1.5, z) for z in zs] + [[np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [1.0, 0.0, 0.0]], dtype=np.float32)
    out, ref = _splat([p], K, (1, 4), mode=mode)
    assert out["count"].tolist() == ([[[0, 6, 0, 0]]] if mode == "nearest" else [[[0, 7, 0, 0]]])      # mean mode keeps z = -1
    out, ref = _splat([p], K, (1, 4), mode=mode, depth_range=(float(lo), float(hi)))
    assert out["count"].tolist() == [[[0, 3, 0, 0]]]
    if mode == "nearest":
        assert out["index"][0, 0, 1] == 6 and out["depth"][0, 0, 1] == lo
    big = np.array([[0.0, 0.0, 2.0 ** 20], [0.0, 0.0, np.nextafter(np.float32(2.0 ** 20), np.float32(2.0 ** 21))], [0.0, 0.0, -2.0 ** 20]], dtype=np.float32)
    out, ref = _splat([big], K, (1, 1), mode=mode)
    assert out["count"].tolist() == ([[[2]]] if mode == "nearest" else [[[2]]])                        # nearest: both positive; mean: |z| <= 2^20
    assert out["depth"][0, 0, 0] == (np.float32(2.0 ** 20) if mode == "nearest" else 0.0)


def test_identity_transform_equals_no_transform():
    clouds, colors, K, _ = _scene(2, CHUNK + 1, (7, 9), seed=9)
    clouds = [np.where(c == 0, np.float32(0.0), c) for c in clouds]                 # 0 * x + ... would turn a -0.0 into +0.0
    for c in clouds:
        c[~np.isfinite(c).all(axis=1)] = [0.1, 0.1, 1.0]                             # and 0 * inf is a NaN
    eye = np.eye(3, 4, dtype=np.float32)[None]
    for mode in ("nearest", "mean"):
        a, _ = _splat(clouds, K, (7, 9), colors=colors, mode=mode)
        b, _ = _splat(clouds, K, (7, 9), colors=colors, mode=mode, T=eye)
        for k in ("depth", "index", "count", "rgb"):
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (mode, k)


@pytest.mark.parametrize("mode", ["nearest", "mean"])
@pytest.mark.parametrize("colour", ["u8", "f32"])
def test_packed_rows_with_an_empty_image_and_overflowed_capacity(mode, colour):
    """an image without rows in the middle; offsets[B] beyond the rows that exist (a PointCloud whose capacity overflowed): the last image
    loses its tail, nothing is read behind n_points"""
    hw, sizes = (7, 9), (700, 0, 900, 0)
    clouds, colors, K, T = _scene(1, 1600, hw, seed=21, f32_colors=colour == "f32")
    clouds, colors = _resplit(clouds, colors, sizes)
    K4 = np.concatenate([K * s for s in (1.0, 1.1, 0.9, 1.2)]).astype(np.float32)
    K4[:, 2, 2] = 1.0
    out, ref = _splat(clouds, K4, hw, layout="packed", colors=colors, mode=mode)
    assert out["count"][1].sum() == 0 and out["count"][3].sum() == 0 and out["count"][0].sum() > 0 and out["count"][2].sum() > 0
    xyz, col = np.concatenate(clouds), np.concatenate(colors)
    offsets = np.array([0, 700, 700, 1600, 1900], dtype=np.int64)                    # 300 rows of image 3 and 100 of image 2 were never written
    n_rows = 1500
    per_image = mg.split_packed(xyz, offsets, n_rows)
    assert [c.shape[0] for c in per_image] == [700, 0, 800, 0]
    ref = mg.restate(per_image, K4, hw, mode=mode, colors=mg.split_packed(col, offsets, n_rows) if mode == "nearest" else None)
    poison = np.full((100, 3), np.nan, dtype=np.float32)
    poison[:, 2] = 0.1                                                               # rows behind n_points: nearer than everything, never read
    out = _call(np.concatenate([xyz[:n_rows], poison]), (0, 3, 1), n_rows, 4, hw, K4, offsets=offsets,
                color=np.concatenate([col[:n_rows], col[:100]]) if mode == "nearest" else None, mode=mode)
    _compare(out, ref, mode)


@pytest.mark.parametrize("colour", ["u8", "f32"])
@pytest.mark.parametrize("layout", ["rows", "planar"])
def test_colours_and_outputs_not_requested(colour, layout):
    clouds, colors, K, T = _scene(2, CHUNK + 1, (7, 9), seed=31, f32_colors=colour == "f32")
    full, _ = _splat(clouds, K, (7, 9), layout=layout, colors=colors, T=T)
    assert full["rgb"].dtype == (np.float32 if colour == "f32" else np.uint8) and (full["index"] >= 0).any()
    bare, _ = _splat(clouds, K, (7, 9), layout=layout, T=T, want_index=False, want_count=False)      # _call checks the untouched outputs
    assert bare["index"] is None and bare["count"] is None and bare["rgb"] is None
    assert np.array_equal(bare["depth"].view(np.uint32), full["depth"].view(np.uint32))
    _splat(clouds, K, (7, 9), layout=layout, T=T, mode="mean", want_count=False)


def test_mean_headroom_is_nan_at_2_pow_19_points():
    N = 2 ** 19
    p = np.zeros((2 * N - 1, 3), dtype=np.float32)
    p[:, 2] = 1.0
    p[N:, 0] = 1.5                                                                    # N points on pixel 0, N - 1 on pixel 1
    out, ref = _splat([p], np.eye(3, dtype=np.float32)[None], (1, 2), mode="mean")
    assert out["count"].tolist() == [[[N, N - 1]]] and np.isnan(out["depth"][0, 0, 0]) and out["depth"][0, 0, 1] == 1.0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------

def test_round_trip_through_pack_points():
    """depth -> pack_points(depth mode) -> render_depth(pixel_offset = 0.5) is the input on its valid pixels and 0 elsewhere, bit for bit"""
    from unidepth_amd import pack_points, render_depth
    B, H, W = 2, 37, 53
    g = np.random.default_rng(41)
    depth = (0.5 + 7.5 * g.random((B, H, W))).astype(np.float32)
    mask = g.random((B, H, W)) < 0.7
    K = np.array([[48.0, 0.0, 26.25], [0.0, 47.5, 18.5], [0.0, 0.0, 1.0]], dtype=np.float32)
    # ud_pointcloud_pack's unprojection restated in fp32 (x = ((u - cx) * d) / fx), then this side's arithmetic: every point must come home
    f32 = np.float32
    vv, uu = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    clouds = []
    for b in range(B):
        x = ((uu - K[0, 2]) * depth[b]) / K[0, 0]
        y = ((vv - K[1, 2]) * depth[b]) / K[1, 1]
        assert x.dtype == f32 and y.dtype == f32
        clouds.append(np.stack([x, y, depth[b]], axis=-1)[mask[b]])
    home = [np.nonzero(mask[b].reshape(-1))[0] for b in range(B)]
    for (pix, _), h in zip(mg.cells(clouds, K, (H, W), pixel_offset=0.5), home):
        assert np.array_equal(pix, h)                                                # 100 % of the points return to their own pixel
    d, m = torch.from_numpy(depth).cuda(), torch.from_numpy(mask).cuda()
    Kd = torch.from_numpy(K).cuda()
    cloud = pack_points(depth=d, intrinsics=Kd, mask=m, capacity=B * H * W, return_index=True)
    view = render_depth(cloud, Kd, (H, W), pixel_offset=0.5, return_index=True, return_count=True)
    want = np.where(mask, depth, f32(0.0))
    assert view.depth.shape == (B, 1, H, W) and view.rgb is None
    assert np.array_equal(view.depth.cpu().numpy()[:, 0].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(view.count.cpu().numpy(), mask.astype(np.int32))
    # the winner's index is its row inside its image: the k-th valid pixel
    rank = np.where(mask, np.cumsum(mask.reshape(B, -1), axis=1).reshape(B, H, W) - 1, -1)
    assert np.array_equal(view.index.cpu().numpy(), rank.astype(np.int32))
    tight = pack_points(depth=d, intrinsics=Kd, mask=m, capacity=int(mask[0].sum()) + 100)           # overflowed: image 1 keeps 100 rows
    part = render_depth(tight, Kd, (H, W), pixel_offset=0.5)
    got = part.depth.cpu().numpy()[:, 0]
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and (got[1] != 0).sum() == 100


def test_render_depth_input_forms_agree_without_host_sync():
    """[B,3,h,w], [B,N,3] and a PointCloud of the same points give the same view; no call synchronises; channels-last inputs are accepted"""
    from unidepth_amd import PointCloud, RenderedView, render_depth
    B, h, w, hw = 2, 20, 30, (17, 23)
    clouds, colors, K, T = _scene(B, h * w, hw, seed=51)
    ref = mg.restate(clouds, K, hw, T=T, colors=colors, depth_range=(0.8, 3.0))
    rows, cols = torch.from_numpy(np.stack(clouds)).cuda(), torch.from_numpy(np.stack(colors)).cuda()
    planar, pcols = rows.permute(0, 2, 1).reshape(B, 3, h, w).contiguous(), cols.permute(0, 2, 1).reshape(B, 3, h, w).contiguous()
    packed = PointCloud(rows.reshape(-1, 3), cols.reshape(-1, 3), None, torch.full((B,), h * w, dtype=torch.int64).cuda(),
                        torch.arange(B + 1, dtype=torch.int64).cuda() * (h * w))
    Kd, Td = torch.from_numpy(K).cuda(), torch.from_numpy(T).cuda()
    T44 = torch.cat([Td, torch.tensor([0.0, 0.0, 0.0, 1.0]).cuda().expand(B, 1, 4)], dim=1)
    work = torch.empty(12 * B * hw[0] * hw[1] + 64, dtype=torch.uint8, device="cuda")
    kw = dict(depth_range=(0.8, 3.0), return_index=True, return_count=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        views = [render_depth(rows, Kd, hw, transform=Td, image=cols, **kw),
                 render_depth(planar, Kd, hw, transform=T44, image=pcols, workspace=work, **kw),
                 render_depth(planar.to(memory_format=torch.channels_last), Kd, hw, transform=Td, image=pcols, **kw),
                 render_depth(packed, Kd, hw, transform=Td, **kw)]                  # the cloud's own rgb
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for v in views:
        assert isinstance(v, RenderedView) and v.depth.shape == (B, 1, *hw) and v.rgb.shape == (B, 3, *hw) and v.rgb.dtype == torch.uint8
        out = {"depth": v.depth.cpu().numpy()[:, 0], "index": v.index.cpu().numpy(), "count": v.count.cpu().numpy(), "rgb": v.rgb.cpu().numpy()}
        _compare(out, ref, "nearest")
    bare = render_depth(rows, Kd[0], hw)
    assert bare.rgb is None and bare.index is None and bare.count is None
    empty = render_depth(PointCloud(torch.empty(0, 3).cuda(), None, None, torch.zeros(B, dtype=torch.int64).cuda(), torch.zeros(B + 1, dtype=torch.int64).cuda()), Kd, hw)
    assert not empty.depth.any()
    with pytest.raises(ValueError):
        render_depth(rows, Kd.cpu(), hw)
    with pytest.raises(ValueError):
        render_depth(rows, Kd, hw, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", list(mg.PP_CASES))
def test_project_points_on_the_golden_cases(name):
    """against the float64 mean by the fixed-point bound, against the reference's fp32 map by that plus the reference's own summation error"""
    from unidepth_amd import project_points
    pts, K, (H, W), _ = mg.pp_inputs(name)
    got = project_points(torch.from_numpy(pts).cuda(), torch.from_numpy(K).cuda(), (H, W))
    assert got.shape == (pts.shape[0], 1, H, W) and got.dtype == torch.float32
    got = got.cpu().numpy()[:, 0].astype(np.float64)
    r = mg.restate(list(pts), K, (H, W), mode="mean", rounding="trunc")
    gold = np.load(mg.GOLDEN)[name][:, 0].astype(np.float64)
    n = r["count"].astype(np.float64)
    assert np.array_equal(got == 0, gold == 0)
    assert (np.abs(got - r["depth"]) <= _mean_bound(r["depth"])).all()
    ref_err = np.maximum(n - 1, 0) * 2.0 ** -24 * r["abs_sum"] / np.maximum(n, 1) + 2.0 ** -24 * np.abs(r["depth"])
    assert (np.abs(got - gold) <= _mean_bound(r["depth"]) + ref_err).all()


@pytest.mark.parametrize("name", list(mg.DS_CASES))
def test_downsample_on_the_golden_cases(name):
    from unidepth_amd import downsample
    data, f = mg.ds_inputs(name)
    got = downsample(torch.from_numpy(data).cuda(), f)
    gold = np.load(mg.GOLDEN)[name]
    assert got.shape == gold.shape and np.array_equal(got.cpu().numpy().view(np.uint32), gold.view(np.uint32))


def test_minpool_guarded_with_nan_and_signed_zero():
    """the C-ABI on a guarded output: more than one tile of output pixels, a NaN block, -0.0 holes, the constants met exactly"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    N, H, W, f = 2, 3 * 18, 3 * 17, 3                                                # 18 x 17 = 306 output pixels per image: two tiles
    g = np.random.default_rng(61)
    d = np.where(g.random((N, 1, H, W)) < 0.8, 0.0, 0.5 + 1200.0 * g.random((N, 1, H, W))).astype(np.float32)
    d[0, 0, 0:3, 0:3] = [[0.0, -0.0, 1000.0], [0.0, 0.0, 2000.0], [-0.0, 0.0, 0.0]]
    d[0, 0, 3:6, 0:3] = [[0.0, 0.0, 1000.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    d[1, 0, 6:9, 3:6] = [[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 0.0]]
    want = mg.restate_minpool(d, f)
    assert want[0, 0, 0, 0] == 1000.0 and want[0, 0, 1, 0] == 0.0 and np.isnan(want[1, 0, 2, 1])
    gd, dst = _guard(want.size, torch.float32)
    src = torch.from_numpy(d).cuda()
    check(_lib.lib.ud_depth_minpool(mk(_lib.UdDepthMinPool, src=src, dst=dst.data_ptr(), N=N, H=H, W=W, factor=f), cur_stream()), "ud_depth_minpool")
    torch.cuda.synchronize()
    gd.check_guards()
    got = dst.cpu().numpy().reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


# ---- end to end: a real infer() output ---------------------------------------------------------------------------------------------

def test_reproject_as_pipeline_post_hook():
    """UniDepthV2 ViT-S (synthetic checkpoint) at 300 x 400, the smallest golden shape of oracle/cases.py: two requests in flight, each
    re-rendering its own output on its own stream right behind infer(): shapes, and the same bits as one at a time.  No numeric claim."""
    from oracle import cases, synth
    from unidepth_amd import UniDepthV2, reproject
    from unidepth_amd.pipeline import InferPipeline
    case = cases.CASES["vits_300x400_eucm"]
    cfg = synth.load_config(case["arch"])
    model = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, case["ckpt_seed"])).to("cuda").eval()
    H, W = case["H"], case["W"]
    rgbs = [torch.randint(0, 256, (1, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(s)).cuda()
            for s in (case["img_seed"], case["img_seed"] + 100)]
    K2 = torch.tensor([[0.8 * W, 0.0, W / 2.0], [0.0, 0.8 * W, H / 2.0], [0.0, 0.0, 1.0]]).cuda()
    T12 = torch.tensor([[1.0, 0.0, 0.0, 0.05], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.1]]).cuda()
    outs = [{k: v.clone() for k, v in model.infer(r).items()} for r in rgbs]
    alone = [reproject(o, K2, T12, image=r, return_index=True) for o, r in zip(outs, rgbs)]
    small = reproject(outs[0], K2, T12, image_shape=(H // 2, W // 2), mode="mean", return_count=True)
    torch.cuda.synchronize()
    assert small.depth.shape == (1, 1, H // 2, W // 2) and small.count.shape == (1, H // 2, W // 2) and small.rgb is None
    pipe = InferPipeline(model, depth=2)
    views = []
    for r in rgbs:
        pipe.submit(r, post=lambda o, r=r: views.append(reproject(o, K2, T12, image=r, return_index=True)))
    pipe.sync()
    assert len(views) == 2
    for a, v in zip(alone, views):
        assert v.depth.shape == (1, 1, H, W) and v.rgb.shape == (1, 3, H, W) and v.rgb.dtype == torch.uint8 and v.index.shape == (1, H, W)
        assert v.count is None
        for x, y in ((a.depth, v.depth), (a.rgb, v.rgb), (a.index, v.index)):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
