"""Surface normals and their metrics without a GPU (unidepth_amd/normals.py, include/unidepth_hip.h UdNormals / UdEvalNormals): the
per-pixel functions of csrc/normals_point.h compiled for the host and run under the host sanitizers (tests/normals_host/normals_host.cpp,
a stand-alone program) against the numpy fp32 restatement of tests/normals_common.py, bit for bit -- the scene with and without the edge
test, the depth form through all six camera models, both known answers, the special values, the rgb bytes; the restatement of the metrics
against a plain float64 formulation; the C-ABI's descriptors, every refusal of the entry points and the Python argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import normals_common as nc

ROOT = nc.ROOT
SIZES = ((nc.H0, nc.W0), (9, 130), (64, 64), (1, 7), (5, 1))


@pytest.fixture(scope="module")
def normals_host(tmp_path_factory):
    return nc.build_host(tmp_path_factory)


@pytest.fixture(scope="module")
def scene_normals(normals_host):
    """the scene's and the prediction's normals through the six models, from the host program: the inputs of the metric tests"""
    d0, m = nc.scene()
    kw = dict(params=nc.rows(nc.MODELS), models=nc.MODELS, mask=m)
    return nc.host_normals(normals_host, depth=d0, **kw)["normals"], nc.host_normals(normals_host, depth=nc.pred_depth(), **kw)["normals"], m


# ---- the per-pixel functions against the restatement, on the host -------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("edge", (None, nc.EDGE_RTOL), ids=("no_edge", "edge"))
def test_host_depth_form_equals_the_restatement(normals_host, size, edge):
    """the depth form through all six models: the program reconstructs the points with camera_models.h (the chain), checks the fused
    order of the kernel against it (exit status 3 otherwise) and its normals, valid and rgb equal the restatement on those points, the
    mask & (depth > 0) and the depth.  The scene's conditions hold at the sizes that can have valid pixels."""
    H, W = size
    depth, mask = nc.scene(H, W)
    h = nc.host_normals(normals_host, depth=depth, params=nc.rows(nc.MODELS), models=nc.MODELS, mask=mask, edge_rtol=edge)
    r = nc.restate_normals(h["points"], (mask[:, 0] != 0) & (depth[:, 0] > 0), depth, edge)
    nc.assert_same(h, r, f"{H}x{W}")
    if min(H, W) == 1:
        assert not r["valid"].any() and not h["normals"].any() and not h["rgb"].any()
    else:
        nc.check_conditions(r, edge is not None)
        assert (np.abs(np.linalg.norm(r["normals"].astype(np.float64), axis=1) - 1)[r["valid"]] < 1e-6).all()
        # every valid normal faces the viewer
        assert ((r["normals"].astype(np.float64) * h["points"]).sum(axis=1)[r["valid"]] <= 0).all()


def test_host_points_form_equals_the_restatement(normals_host):
    """the points form on the scene's points: without a depth the edge test compares z, with a shared mask and with none"""
    depth, mask = nc.scene()
    pts = nc.host_normals(normals_host, depth=depth, params=nc.rows(nc.MODELS), models=nc.MODELS)["points"]
    for kw in (dict(mask=mask), dict(mask=mask, edge_rtol=nc.EDGE_RTOL), dict(mask=mask, depth=depth, edge_rtol=nc.EDGE_RTOL),
               dict(mask=mask[:1], edge_rtol=0.0), dict()):
        h = nc.host_normals(normals_host, points=pts, **kw)
        r = nc.restate_normals(pts, kw.get("mask"), kw.get("depth"), kw.get("edge_rtol"))
        nc.assert_same(h, r, str(sorted(kw)))
        if kw.get("edge_rtol") != 0.0:                  # a tolerance of 0 keeps only neighbours of exactly the same z
            assert 0.3 < r["valid"].mean() < 0.99          # without a mask only the NaN points drop out


def test_host_known_answers(normals_host):
    def run(pts):
        h = nc.host_normals(normals_host, points=pts)
        nc.assert_same(h, nc.restate_normals(pts), "known answer")
        return h["normals"], h["valid"]
    nc.check_known_answer(run)
    # the rgb bytes of (0, 0, -1): floor(127.5 + 0.5) = 128, 128, floor(0 + 0.5) = 0
    h = nc.host_normals(normals_host, points=nc.known_answers()[0][0])
    assert (h["rgb"][:, 0] == 128).all() and (h["rgb"][:, 1] == 128).all() and (h["rgb"][:, 2] == 0).all()


def test_host_special_values(normals_host):
    """depth 0, -0.0, negative, NaN, +-inf and 1e-30 at the head of the first rows; points of 1e30 (overflow), neighbours 1e-30 apart
    (underflow to m = 0), coincident neighbours, and mirrored clouds whose normals take the flip branch"""
    depth, mask = nc.special_depth(), nc.scene()[1]
    for edge in (None, nc.EDGE_RTOL):
        h = nc.host_normals(normals_host, depth=depth, params=nc.rows(nc.MODELS), models=nc.MODELS, mask=mask, edge_rtol=edge)
        r = nc.restate_normals(h["points"], (mask[:, 0] != 0) & (depth[:, 0] > 0), depth, edge)
        nc.assert_same(h, r, "special depth")
        assert not r["valid"][:, 0, 0:3].any() and not r["valid"][:, 1, 1:3].any()          # 0, negative, NaN / -inf, -0.0
    pts = nc.special_points()
    for kw in (dict(), dict(edge_rtol=0.5)):
        h = nc.host_normals(normals_host, points=pts, **kw)
        r = nc.restate_normals(pts, None, None, kw.get("edge_rtol"))
        nc.assert_same(h, r, "special points")
    r = nc.restate_normals(pts)
    assert not r["valid"][0].any() and not r["valid"][1].any()                               # overflow, underflow
    assert not r["valid"][2, 3, 4:6].any() and r["valid"][2].sum() > 40                      # the inside of the coincident block
    assert not r["valid"][2, 6, 2] and not r["valid"][2, 6, 6] and not r["valid"][2, 7, 8]   # NaN, inf, -inf coordinates
    for b in (3, 4):                                                                         # mirrored: valid, facing the viewer, flipped
        assert r["valid"][b].all()
        assert ((r["normals"][b].astype(np.float64) * pts[b]).sum(axis=0) <= 0).all()
        assert r["flipped"][b].sum() >= 0.5 * r["valid"][b].sum()


# ---- the restatement of the metrics -------------------------------------------------------------------------------------------------

def test_metric_restatement_against_the_plain_formulation(scene_normals):
    """the fp32 cosine and its float64 acos against arccos of the float64 normalised dot product.  The cosine carries at most 7 fp32
    roundings (three products and two sums of the dot behind the lengths' own, a product, a quotient): |dc| <= 7 * 2^-24 = 4.2e-7, and
    acos moves by at most sqrt(2 |dc|) = 9.2e-4 rad = 0.053 degrees (the worst case, at c = 1).  Counts are equal on these inputs."""
    gt, pred, mask = scene_normals
    r, p = nc.restate_eval(gt, pred, mask), nc.plain_eval(gt, pred, mask)
    assert (r["count"] == p["count"]).all() and (r["count"] > 1000).all()
    for t in nc.THRESHOLDS:
        assert (r[f"n_{t}"] == p[f"n_{t}"]).all(), t
        # the amplitude of the prediction's noise was chosen for this: every share of every image inside (0.05, 0.95)
        assert (r[f"a_{t}"] > 0.05).all() and (r[f"a_{t}"] < 0.95).all(), (t, r[f"a_{t}"])
    for k in ("mean", "median", "rmse"):
        assert np.abs(r[k] - p[k]).max() <= 0.053, (k, r[k], p[k])


def test_metric_restatement_special_cases():
    g = np.zeros((4, 3, 2, 3), np.float32)
    g[:, 2] = -1.0
    p = g.copy()
    p[1] = -p[1]                                        # opposite: 180
    p[2, :, 0, 0] = [0.0, -1.0, 0.0]                    # one pixel at 90
    g[3, :, :, :] = np.nan                              # no usable pixel
    r = nc.restate_eval(g, p)
    assert r["mean"][0] == 0 and r["mean"][1] == 180 and r["median"][1] == 180 and r["rmse"][1] == 180
    assert r["median"][2] == 0 and abs(r["mean"][2] - 15.0) < 1e-12
    assert r["count"].tolist() == [6, 6, 6, 0] and np.isnan(r["mean"][3]) and np.isnan(r["a_11.25"][3])
    assert r["a_11.25"][0] == 1 and r["a_11.25"][1] == 0
    # the lower median of two: the smaller error
    g2 = np.zeros((1, 3, 1, 2), np.float32)
    g2[:, 2] = 1.0
    p2 = g2.copy()
    p2[0, :, 0, 1] = [1.0, 0.0, 0.0]
    assert nc.restate_eval(g2, p2)["median"][0] == 0


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------

def test_eval_normals_takes_at_most_eight_thresholds():
    from unidepth_amd import _lib
    assert _lib.UD_EVAL_NORMALS_MAX_T == 8


def test_every_refusal_of_ud_normals():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_normals(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()

    def call(**kw):
        d = _lib.UdNormals()
        base = dict(points=None, depth=16, params=16, mask=None, normals=16, valid=None, rgb=None, B=2, H=4, W=6, mask_shared=0, has_rtol=0,
                    rtol_bits=0)
        base.update(kw)
        models = base.pop("models", (1, 6))
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(models):
            d.model[b] = m
        return lib.ud_normals(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg, rc_want in (
            (dict(B=0), "bad sizes", -1), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes", -1), (dict(H=0), "bad sizes", -1), (dict(W=-1), "bad sizes", -1),
            (dict(H=1 << 16, W=1 << 15), "bad sizes", -1), (dict(H=1, W=2 ** 31 - 256), "bad sizes", -1), (dict(H=524281, W=1), "bad sizes", -1),
            (dict(normals=None), "null pointer", -1), (dict(depth=None), "null pointer", -1), (dict(params=None), "null pointer", -1),
            (dict(has_rtol=1, rtol_bits=nc.f32_bits(-0.5)), "edge_rtol", -1), (dict(has_rtol=1, rtol_bits=nc.f32_bits(float("inf"))), "edge_rtol", -1),
            (dict(has_rtol=1, rtol_bits=nc.f32_bits(float("nan"))), "edge_rtol", -1),
            (dict(models=(0, 1)), "model tag", -1), (dict(models=(1, 7)), "model tag", -1),
            (dict(models=(4, 1)), "iterative model", -3), (dict(models=(1, 5)), "iterative model", -3)):
        rc, err = call(**kw)
        assert rc == rc_want and msg in err, (kw, rc, err)


def test_every_refusal_of_ud_eval_normals():
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_eval_normals(None, 16, 1 << 30, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    need = lib.ud_eval_normals_work_bytes(2, 4, 6, 3)
    assert need > 0 and lib.ud_eval_normals_work_bytes(2, 4, 6, 8) == need
    for bad in ((0, 4, 6, 3), (_lib.UD_RECON_MAX_B + 1, 4, 6, 3), (2, 0, 6, 3), (2, 4, -1, 3), (2, 1 << 16, 1 << 15, 3), (2, 4, 6, 0), (2, 4, 6, 9)):
        assert lib.ud_eval_normals_work_bytes(*bad) == -1, bad

    def call(work=256, nbytes=need, **kw):
        d = _lib.UdEvalNormals()
        base = dict(gt=16, pred=16, mask=None, out=16, count=16, error=None, B=2, H=4, W=6, T=3, mask_shared=0)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.ud_eval_normals(C.byref(d), work, nbytes, None), lib.ud_last_error().decode()
    for kw, msg in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"),
                    (dict(H=1 << 16, W=1 << 15), "bad sizes"), (dict(T=0), "bad sizes"), (dict(T=9), "bad sizes"),
                    (dict(gt=None), "null pointer"), (dict(pred=None), "null pointer"), (dict(out=None), "null pointer"),
                    (dict(count=None), "null pointer"), (dict(work=None), "null pointer"), (dict(work=264), "16-byte aligned"),
                    (dict(nbytes=need - 1), "workspace smaller")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, normals
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    pts, depth = torch.rand(2, 3, 4, 6), torch.rand(2, 1, 4, 6) + 1
    f = normals.normals_from_points
    for bad in (torch.rand(2, 2, 4, 6), torch.rand(2, 24, 3), torch.ones(2, 3, 4, 6, dtype=torch.int32), torch.rand(0, 3, 4, 6), "points"):
        with pytest.raises(ValueError, match="points"):
            f(bad)
    for bad in (torch.ones(2, 1, 4, 5, dtype=torch.bool), torch.ones(2, 4, 6), torch.ones(3, 4, 6, dtype=torch.bool), torch.ones(2, 2, 4, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask"):
            f(pts, mask=bad)
    for bad in (torch.rand(2, 1, 4, 5), torch.ones(2, 4, 6, dtype=torch.bool), torch.rand(1, 4, 6), "depth"):
        with pytest.raises(ValueError, match="depth"):
            f(pts, depth=bad)
    with pytest.raises(ValueError, match="at most"):
        f(torch.rand(257, 3, 1, 1))
    g = normals.normals_camera
    for bad in (torch.rand(2, 2, 4, 6), torch.rand(4, 6), torch.ones(2, 1, 4, 6, dtype=torch.int64), torch.rand(0, 1, 4, 6), "depth"):
        with pytest.raises(ValueError, match="depth"):
            g(bad, K)
    with pytest.raises(ValueError, match="mask"):
        g(depth, K, mask=torch.ones(2, 4, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="at most"):
        g(torch.rand(257, 1, 1, 1), K)
    for bad in (-0.1, float("nan"), float("inf"), 1e300, "tol"):
        with pytest.raises(ValueError, match="edge_rtol"):
            f(pts, edge_rtol=bad)
        with pytest.raises(ValueError, match="edge_rtol"):
            g(depth, K, edge_rtol=bad)
    e = normals.eval_normals
    for bad in (torch.rand(2, 2, 4, 6), torch.ones(2, 3, 4, 6, dtype=torch.int32), torch.rand(0, 3, 4, 6), "gt"):
        with pytest.raises(ValueError, match="gt"):
            e(bad, pts)
        with pytest.raises(ValueError, match="pred"):
            e(pts, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        e(pts, torch.rand(2, 3, 4, 7))
    with pytest.raises(ValueError, match="mask"):
        e(pts, pts, torch.ones(2, 4, 6))
    for bad in ((), tuple(range(1, 10)), (0.0,), (181.0,), (float("nan"),), ("a",), 5):
        with pytest.raises(ValueError, match="thresholds"):
            e(pts, pts, thresholds=bad)
    # well-formed arguments on the CPU: the HIP kernels are the only implementation
    eucm = cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))
    opencv = cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12))
    m = torch.ones(1, 1, 4, 6, dtype=torch.bool)
    for call in (lambda: f(pts), lambda: f(pts, mask=m, depth=depth, edge_rtol=0.05, return_mask=True, return_rgb=True),
                 lambda: g(depth, K), lambda: g(depth[:, 0], eucm, mask=m, edge_rtol=0.1), lambda: g(depth, opencv, return_rgb=True),
                 lambda: g(depth, cameras.BatchCamera([cameras.Pinhole(K), eucm])),
                 lambda: e(pts, pts), lambda: e(pts, pts, m, thresholds=(5.0,), return_error=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    for name in ("normals_from_points", "normals_camera", "eval_normals"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(normals, name)
    assert unidepth_amd._NORMALS == ("normals_from_points", "normals_camera", "eval_normals")
    assert "no valid pixel" in f.__doc__ and "ONE launch" in g.__doc__ and "lower median" in e.__doc__
