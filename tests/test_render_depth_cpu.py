"""Splatting without a GPU (unidepth_amd/reproject.py, include/unidepth_hip.h UdSplat / UdDepthMinPool): the numpy restatement of
tools/make_golden_render_depth.py against the reference's own arrays (tests/golden/render_depth.npz), the C-ABI's argument
checks and workspace query, and the argument errors of render_depth / project_points / downsample / reproject."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_render_depth", os.path.join(ROOT, "tools", "make_golden_render_depth.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


def test_golden_has_every_case():
    g = np.load(mg.GOLDEN)
    assert sorted(g.files) == sorted(list(mg.PP_CASES) + [n + "_cell" for n in mg.PP_CASES] + list(mg.DS_CASES))
    for name, (B, N, H, W, _) in mg.PP_CASES.items():
        assert g[name].dtype == np.float32 and g[name].shape == (B, 1, H, W)
        assert g[name + "_cell"].dtype == np.int32 and g[name + "_cell"].shape == (B, N)
    for name, (N, H, W, f) in mg.DS_CASES.items():
        assert g[name].dtype == np.float32 and g[name].shape == (N, 1, H // f, W // f)
    assert os.path.getsize(mg.GOLDEN) < 64 * 1024


@pytest.mark.parametrize("name", list(mg.PP_CASES))
def test_restatement_matches_reference_project_points(name):
    """every point in the reference's own cell, hence equal counts and holes; the means within the reference's own fp32 summation error
    of the float64 mean: n - 1 additions of relative error 2^-24 each on partial sums of at most sum|z|, and one division"""
    pts, K, (H, W), aimed = mg.pp_inputs(name)
    g = np.load(mg.GOLDEN)
    ref, ref_cell = g[name].astype(np.float64)[:, 0], g[name + "_cell"]
    pix = np.stack([c[0] for c in mg.cells(list(pts), K, (H, W), rounding="trunc")])
    np.testing.assert_array_equal(pix, ref_cell)
    # the inputs were aimed at cells; -1 truncates into 0, as the reference's .int() does
    tu, tv = (np.where(aimed[..., k] == -1, 0, aimed[..., k]) for k in (0, 1))
    np.testing.assert_array_equal(pix, np.where((tu >= 0) & (tu < W) & (tv >= 0) & (tv < H), tv * W + tu, -1))
    assert (pix >= 0).any() and (pix < 0).any() and ((aimed == -1).any(axis=-1) & (pix >= 0)).any()
    r = mg.restate(list(pts), K, (H, W), mode="mean", rounding="trunc")
    n = r["count"].astype(np.float64)
    np.testing.assert_array_equal(r["count"], np.stack([np.bincount(c[c >= 0], minlength=H * W).reshape(H, W) for c in ref_cell]))
    np.testing.assert_array_equal(n == 0, ref == 0)
    bound = np.maximum(n - 1, 0) * 2.0 ** -24 * r["abs_sum"] / np.maximum(n, 1) + 2.0 ** -24 * np.abs(r["depth"])
    err = np.abs(r["depth"] - ref)
    assert (err <= bound).all(), (float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    assert n.max() >= 5 and (pts[..., 2] < 0).any()                 # several points per pixel, and negative depths among them


def test_restatement_nearest_and_edges_by_hand():
    """hand-made points: the winner and its tie-break, z <= 0 / NaN / inf / w = 0, u on cell edges under floor and trunc, the offset,
    the range ends, and the transform"""
    K = np.array([[2.0, 0, 0], [0, 2.0, 0], [0, 0, 1.0]], dtype=np.float32)        # u = 2 x / z
    W, H = 4, 1
    P = lambda u, z=1.0: [u * z / 2.0, 0.0, z]                                      # noqa: E731
    pts = np.array([P(1.5, 3.0), P(1.25, 2.0), P(1.75, 2.0), P(1.5, -1.0), P(1.5, 0.0), P(1.5, np.nan), P(1.5, np.inf),
                    P(0.0), P(-0.0), P(-0.5), P(4.0 - 2.0 ** -20), P(4.0), P(3.5, 5.0)], dtype=np.float32)
    pts[8, 0] = -0.0
    r = mg.restate([pts], K, (H, W), colors=[np.arange(39, dtype=np.uint8).reshape(13, 3)])
    assert r["index"].tolist() == [[[7, 1, -1, 10]]] and r["depth"].tolist() == [[[1.0, 2.0, 0.0, 1.0]]]
    assert r["count"].tolist() == [[[2, 3, 0, 2]]]                                  # floor: u = -0.0 stays, -0.5 and 4.0 leave
    assert r["rgb"][0, :, 0, 1].tolist() == [3, 4, 5] and r["rgb"][0, :, 0, 2].tolist() == [0, 0, 0]
    t = mg.restate([pts], K, (H, W), rounding="trunc")
    assert t["count"].tolist() == [[[3, 3, 0, 2]]]                                  # trunc: u = -0.5 lands in column 0
    o = mg.restate([pts], K, (H, W), pixel_offset=0.5)
    assert o["count"].tolist() == [[[3, 1, 2, 0]]]                                  # -0.5 -> 0, 0 -> 0.5, 1.25 -> 1.75, 1.5 -> 2, 1.75 -> 2.25, 3.5 -> 4 (out)
    d = mg.restate([pts], K, (H, W), depth_range=(2.0, 3.0))
    assert d["count"].tolist() == [[[0, 3, 0, 0]]] and d["depth"].tolist() == [[[0.0, 2.0, 0.0, 0.0]]]
    m = mg.restate([pts], K, (H, W), mode="mean")
    assert m["count"].tolist() == [[[2, 4, 0, 2]]] and m["depth"][0, 0].tolist() == [1.0, 1.5, 0.0, 3.0]   # z = -1 counts; z = 0 gives u = 0 / 0
    T = np.array([[1.0, 0, 0, 0.5], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0]], dtype=np.float32)                    # x + 0.5, z + 1
    s = mg.restate([np.array([[0.0, 0.0, 1.0]], dtype=np.float32)], K, (H, W), T=T)                         # u = 2 * 0.5 / 2 = 0.5
    assert s["index"].tolist() == [[[0, -1, -1, -1]]] and s["depth"].tolist() == [[[2.0, 0.0, 0.0, 0.0]]]


@pytest.mark.parametrize("name", list(mg.DS_CASES))
def test_minpool_restatement_matches_reference_golden(name):
    data, f = mg.ds_inputs(name)
    got, ref = mg.restate_minpool(data, f), np.load(mg.GOLDEN)[name]
    assert got.dtype == ref.dtype and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_minpool_restatement_constants():
    d = np.array([[[[0.0, 0.0, 1000.0, 0.0], [0.0, -0.0, 0.0, 1000.5], [1000.5, 0.0, 3.0, np.nan], [0.0, 2000.0, 0.0, 1.0]]]], dtype=np.float32)
    got = mg.restate_minpool(d, 2)
    assert got[0, 0, 0].tolist() == [0.0, 1000.0] and got[0, 0, 1, 0] == 0.0 and np.isnan(got[0, 0, 1, 1])


@pytest.mark.skipif(not os.path.isfile(mg.reference_path()), reason="reference tree not present (authoring machine only)")
def test_reference_rerun_reproduces_golden():
    out = mg.reference_outputs(mg.reference_module())
    g = np.load(mg.GOLDEN)
    for name in mg.DS_CASES:
        assert np.array_equal(out[name].view(np.uint32), g[name].view(np.uint32)), name
    for name in mg.PP_CASES:
        np.testing.assert_array_equal(out[name + "_cell"], g[name + "_cell"], err_msg=name)
        # the means are fp32 sums in scatter order: equal up to that order's rounding (n <= 32 points per pixel of |z| < 7)
        np.testing.assert_allclose(out[name], g[name], rtol=0, atol=32 * 7 * 2.0 ** -24, err_msg=name)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------

def test_splat_rejects_bad_descriptors_without_a_launch():
    """every refusal comes back before any HIP call: this runs on a machine without a GPU, the pointers are never followed"""
    from unidepth_amd import _lib
    lib = _lib.lib
    P = 0x1000                                      # stands for a device pointer
    B, H, W = 2, 5, 7
    nbytes = lib.ud_splat_work_bytes(B, H, W)

    def rc(**kw):
        base = dict(xyz=P, K=P, depth=P, work=P, work_bytes=nbytes, batch_stride=30, point_stride=3, comp_stride=1, n_points=10,
                    B=B, H=H, W=W, nK=1, mode=_lib.UD_SPLAT_NEAREST)
        base.update(kw)
        d = _lib.UdSplat()
        for k, v in base.items():
            setattr(d, k, v)
        r = lib.ud_splat(C.byref(d), None)
        return r, lib.ud_last_error().decode()

    r, msg = lib.ud_splat(None, None), lib.ud_last_error().decode()
    assert r < 0 and "null descriptor" in msg
    MEAN = _lib.UD_SPLAT_MEAN
    for kw, word in ((dict(B=0), "bad sizes"), (dict(B=65536), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-1), "bad sizes"),
                     (dict(H=65536, W=65536, work_bytes=1 << 60), "bad sizes"),
                     (dict(n_points=-1), "bad sizes"), (dict(n_points=1 << 31), "bad sizes"),
                     (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"),
                     (dict(flags=4), "unknown flag"),
                     (dict(xyz=None), "null pointer"), (dict(depth=None), "null pointer"),
                     (dict(point_stride=0), "bad strides"), (dict(comp_stride=0), "bad strides"), (dict(batch_stride=-1), "bad strides"),
                     (dict(K=None), "K [nK,3,3]"), (dict(nK=0), "K [nK,3,3]"), (dict(nK=3), "K [nK,3,3]"),
                     (dict(T=P, nT=0), "nT"), (dict(T=P, nT=3), "nT"),
                     (dict(color=P), "color and rgb"), (dict(rgb=P), "color and rgb"),
                     (dict(mode=MEAN, index=P), "UD_SPLAT_NEAREST only"), (dict(mode=MEAN, color=P, rgb=P), "UD_SPLAT_NEAREST only"),
                     (dict(work=None), "work is null"), (dict(work=P + 4), "work is null"),
                     (dict(work_bytes=B * H * W * 8 - 1), "work is null"),
                     (dict(work_bytes=B * H * W * 12 - 1, count=P), "work is null"),
                     (dict(work_bytes=B * H * W * 12 - 1, mode=MEAN), "work is null")):
        r, msg = rc(**kw)
        assert r < 0 and word in msg, (kw, r, msg)


def test_minpool_rejects_bad_descriptors_without_a_launch():
    from unidepth_amd import _lib
    lib = _lib.lib
    P = 0x1000

    def rc(**kw):
        base = dict(src=P, dst=P, N=2, H=12, W=16, factor=2)
        base.update(kw)
        d = _lib.UdDepthMinPool()
        for k, v in base.items():
            setattr(d, k, v)
        r = lib.ud_depth_minpool(C.byref(d), None)
        return r, lib.ud_last_error().decode()

    r, msg = lib.ud_depth_minpool(None, None), lib.ud_last_error().decode()
    assert r < 0 and "null descriptor" in msg
    for kw, word in ((dict(factor=0), "factor"), (dict(factor=65, H=65, W=65), "factor"), (dict(factor=5), "bad sizes"),
                     (dict(factor=3), "bad sizes"), (dict(N=0), "bad sizes"), (dict(N=65536), "bad sizes"), (dict(H=0), "bad sizes"),
                     (dict(H=65536, W=65536), "bad sizes"), (dict(src=None), "null pointer"), (dict(dst=None), "null pointer")):
        r, msg = rc(**kw)
        assert r < 0 and word in msg, (kw, r, msg)


def test_work_bytes_bounds_and_monotonicity():
    from unidepth_amd import _lib
    wb = _lib.lib.ud_splat_work_bytes
    for B, H, W in ((1, 1, 1), (1, 7, 9), (3, 37, 53), (8, 518, 518), (8, 480, 640), (65535, 32768, 65535)):
        n = wb(B, H, W)
        assert n == B * H * W * 12                             # 8 B per pixel for the key / sum, 4 B for the count
        if B < 65535:
            assert wb(B + 1, H, W) > n and wb(B, H + 1, W) > n and wb(B, H, W + 1) > n
    assert wb(0, 4, 4) < 0 and wb(1, 0, 4) < 0 and wb(1, 4, -1) < 0 and wb(1, 65536, 32768) < 0 and wb(65536, 4, 4) < 0
    assert wb(1, 1, 2 ** 31 - 1) == (2 ** 31 - 1) * 12


# ---- argument errors of the Python surface (CPU tensors: every check comes before any launch) ---------------------------------------

def test_render_depth_argument_errors():
    from unidepth_amd import PointCloud, downsample, project_points, render_depth, reproject
    pts = torch.zeros(2, 3, 6, 8)
    rows = torch.zeros(2, 50, 3)
    K = torch.eye(3)
    cloud = PointCloud(torch.zeros(20, 3), torch.zeros(20, 3, dtype=torch.uint8), None, torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    bad = [
        dict(points=torch.zeros(2, 4, 6, 8)),                                     # shapes
        dict(points=torch.zeros(2, 50, 2)),
        dict(points=torch.zeros(50, 3)),
        dict(points=pts.double()),                                                # dtypes
        dict(points=[[0.0, 0.0, 1.0]]),
        dict(points=pts, intrinsics=torch.eye(3).expand(3, 3, 3)),                # nK not 1 or B
        dict(points=pts, intrinsics=torch.eye(3).double()),
        dict(points=pts, intrinsics=torch.eye(4)),
        dict(points=pts, image_shape=(6,)),
        dict(points=pts, image_shape=(0, 8)),
        dict(points=pts, image_shape=5),
        dict(points=pts, transform=torch.eye(3)),
        dict(points=pts, transform=torch.eye(4).expand(3, 4, 4)),
        dict(points=pts, mode="max"),
        dict(points=pts, rounding="round"),
        dict(points=pts, depth_range=5.0),
        dict(points=pts, depth_range=(1.0, 2.0, 3.0)),
        dict(points=pts, image=torch.zeros(2, 3, 6, 7, dtype=torch.uint8)),       # image not shaped like the points
        dict(points=rows, image=torch.zeros(2, 3, 5, 10, dtype=torch.uint8)),
        dict(points=pts, image=torch.zeros(2, 3, 6, 8, dtype=torch.float16)),
        dict(points=pts, image=torch.zeros(2, 3, 6, 8), mode="mean"),
        dict(points=pts, return_index=True, mode="mean"),
        dict(points=cloud, image=torch.zeros(19, 3, dtype=torch.uint8)),
        dict(points=PointCloud(torch.zeros(20, 3), None, None, torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32))),
        dict(points=pts),                                                         # CPU tensors: there is no CPU path
        dict(points=rows),
        dict(points=cloud),
    ]
    for kw in bad:
        kw = dict(dict(intrinsics=K, image_shape=(6, 8)), **kw)
        with pytest.raises(ValueError):
            render_depth(kw.pop("points"), kw.pop("intrinsics"), kw.pop("image_shape"), **kw)
    with pytest.raises(ValueError):
        reproject({"depth": pts[:, :1]}, K)
    with pytest.raises(ValueError):
        reproject({"points": pts}, K)                                             # CPU
    for args in ((torch.zeros(2, 50, 2), K[None].expand(2, 3, 3), (6, 8)), (rows, K[None].expand(3, 3, 3), (6, 8)), (rows, K[None].expand(2, 3, 3), (6, 8))):
        with pytest.raises(ValueError):
            project_points(*args)
    for args in ((torch.zeros(2, 1, 6, 8), 4), (torch.zeros(2, 1, 6, 8), 0), (torch.zeros(2, 1, 6, 8), 2.0), (torch.zeros(2, 3, 6, 8), 2),
                 (torch.zeros(2, 6, 8), 2), (torch.zeros(2, 1, 6, 8).double(), 2), (torch.zeros(2, 1, 6, 8), 2)):
        with pytest.raises(ValueError):
            downsample(*args)


def test_lazy_exports():
    import unidepth_amd
    from unidepth_amd import reproject as module
    for name in ("RenderedView", "render_depth", "project_points", "downsample"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(module, name)
    # the function reproject() shares its name with its module: whichever the package attribute is bound to, a call reaches the function
    assert "reproject" in unidepth_amd.__all__ and callable(unidepth_amd.reproject) and callable(module.reproject)
    with pytest.raises(ValueError, match="no 'points'"):
        unidepth_amd.reproject({}, torch.eye(3))
