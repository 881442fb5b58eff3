"""Camera.project / project_camera / render_depth_camera without a GPU (unidepth_amd/reproject.py, unidepth_amd/cameras.py,
include/unidepth_hip.h UdCameraProject / UdSplatCamera): the numpy fp32 restatement of tools/make_golden_camera_project.py against the
reference's own Camera.project arrays (tests/golden/camera_project.npz) at the measured bars, the conditions the generator promises,
the forward models of csrc/camera_models.h compiled for the host (tests/proj_host/proj_host.cpp, a stand-alone program), the golden
pinned to the live reference where it is present, the C-ABI's descriptors and refusals and the Python argument errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import camera_project_common as common
import host_program

ROOT = common.ROOT
cp, gp = common.cp, common.gp
_case, _bars = common.case, common.bars


def test_golden_has_every_case():
    g = common.golden()
    want = [f"{n}.{k}" for n in cp.CASES for k in ("xyz", "params", "models", "uv", "mask", "n_regular")]
    want += ["referr." + n for n in cp.MODEL_NAMES.values()] + ["roundtrip"]
    assert sorted(g) == sorted(want)
    assert set(cp.CASES) == set(gp.CASES)
    for name in cp.CASES:
        c = _case(name)
        B, N = len(c["models"]), c["H"] * c["W"]
        # the seeded inputs are the stored ones, bit for bit (NaN included)
        assert c["xyz"].shape == (B, N, 3) and np.array_equal(g[name + ".xyz"].view(np.uint32), c["xyz"].view(np.uint32))
        assert np.array_equal(g[name + ".params"], c["params"]) and list(g[name + ".models"]) == c["models"]
        assert np.array_equal(g[name + ".params"], gp.case_rows(name)[1])              # the camera rows of the gt_points cases
        assert g[name + ".uv"].dtype == np.float32 and g[name + ".uv"].shape == (B, 2, c["H"], c["W"])
        assert g[name + ".mask"].dtype == np.uint8 and g[name + ".mask"].shape == (B, 1, c["H"], c["W"])
        assert int(g[name + ".n_regular"]) == c["n_reg"] >= 20
    assert os.path.getsize(cp.GOLDEN) < 1024 * 1024
    assert sorted(g["roundtrip"]) == sorted(cp.roundtrip_cases())
    covered = {m for n in g["roundtrip"] for m in _case(str(n))["models"]}
    assert covered == set(cp.MODEL_NAMES), "the round trip must reach every model"


def test_regular_points_are_well_conditioned_and_special_points_are_there():
    for name in cp.CASES:
        c = _case(name)
        n = c["n_reg"]
        for b, m in enumerate(c["models"]):
            assert cp.well_conditioned(c["xyz"][b, :n], c["params"][b], m, (c["H"], c["W"])).all(), (name, b)
            assert np.array_equal(c["in32"][b, :n], c["in64"][b, :n])
            sp = c["xyz"][b, n:]
            assert np.array_equal(np.nan_to_num(sp, nan=-7.0), np.nan_to_num(cp.SPECIAL[:len(sp)], nan=-7.0))
        if c["H"] * c["W"] > 100:
            sp = c["xyz"][0, n:]
            assert len(sp) == len(cp.SPECIAL) and (sp[:, 2] == 0).any() and (sp[:, 2] < 0).any() and np.isnan(sp).any() and np.isinf(sp).any()
            assert ((sp[:, 0] == 0) & (sp[:, 1] == 0) & (sp[:, 2] > 0)).any()
            # regular points on both sides of the image's border
            assert c["in64"][:, :n].any() and not c["in64"][:, :n].all(), name
    worst = max(cp.bar(float(common.golden()["referr." + n])) for n in cp.MODEL_NAMES.values())
    assert cp.MARGIN >= 8 * worst * 66.0                      # 66 px: 1.25 x the widest image (well_conditioned's spread)


@pytest.mark.parametrize("name", list(cp.CASES))
def test_fp32_restatement_within_measured_bar_of_reference(name):
    c, g, bars = _case(name), common.golden(), _bars()
    ref = common.rows_of(g[name + ".uv"])
    n = c["n_reg"]
    for b, m in enumerate(c["models"]):
        e = cp.uv_error(c["uv32"][b, :n].astype(np.float64) - ref[b, :n], c["uv64"][b, :n])
        assert e.max() <= bars[m], (name, b, e.max(), bars[m])
        # the reference's own masks on the regular points are the restatement's (Pinhole inverted, Spherical none)
        assert np.array_equal(g[name + ".mask"][b].reshape(-1)[:n], cp.class_mask(m, c["in32"][b])[:n])


def test_bars_come_from_the_reference_error():
    g = common.golden()
    worst = {}
    for name in cp.CASES:
        c = _case(name)
        n = c["n_reg"]
        e = cp.uv_error(common.rows_of(g[name + ".uv"])[:, :n].astype(np.float64) - c["uv64"][:, :n], c["uv64"][:, :n])
        for b, m in enumerate(c["models"]):
            worst[m] = max(worst.get(m, 0.0), float(e[b].max()))
    for m, n in cp.MODEL_NAMES.items():
        e = float(g["referr." + n])
        assert 0 < e < 1e-4 and cp.bar(e) == max(4 * e, 8 * 2.0 ** -24)
        assert abs(worst[m] - e) <= 1e-6 * e + 1e-12, n     # the fp64 restatement's libm may differ in its last bit
    txt = open(cp.BARS_TXT).read()
    for n in cp.MODEL_NAMES.values():
        assert f"{float(g['referr.' + n]):.3e}" in txt


def _reference_available():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return ref_loader.available()


@pytest.mark.skipif(not _reference_available(), reason="reference tree not present (authoring machine only)")
def test_reference_rerun_reproduces_golden():
    rc = gp.reference_module()
    g = common.golden()
    for name in cp.CASES:
        uv, mask = cp.reference_output(rc, name)
        assert common.same_bits(uv, g[name + ".uv"]) and np.array_equal(mask, g[name + ".mask"]), name


# ---- the forward models of the header, compiled for the host ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def proj_host(tmp_path_factory):
    out = host_program.build(tmp_path_factory, "proj_host", sanitize=False)

    def run(model, H, W, row, xyz):
        n = len(xyz)
        uv, depth, inside = host_program.run(out, [model, H, W, n] + [float(v).hex() for v in row], [np.ascontiguousarray(xyz, np.float32).tobytes()],
                                             [8 * n, 4 * n, n])
        return np.frombuffer(uv, np.float32).reshape(n, 2), np.frombuffer(depth, np.float32), np.frombuffer(inside, np.uint8).astype(bool)
    return run


@pytest.mark.parametrize("name", list(cp.CASES))
def test_header_functions_on_the_host(proj_host, name):
    """ud_cam_project_<model> / ud_cam_inside / ud_cam_depth over every regular and special point: bit-equal to the fp32 restatement for
    Pinhole, EUCM, OPENCV and MEI, within the measured bar for Spherical and Fisheye624 (atan2f, asinf, atanf differ between libraries)"""
    c, bars = _case(name), _bars()
    uv, depth, inside = [], [], []
    for b, m in enumerate(c["models"]):
        u, d, i = proj_host(m, c["H"], c["W"], c["params"][b], c["xyz"][b])
        uv.append(u), depth.append(d), inside.append(i)
    w = common.assert_uv(np.stack(uv), c, bars, name)
    assert common.same_bits(np.stack(depth), c["d32"])
    assert np.array_equal(np.stack(inside), c["in32"])
    print(f"{name}: host build uses {w:.3f} of the bar")


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_splat_descriptors_differ_in_the_projector_fields_only():
    from unidepth_amd import _lib
    assert _lib.UD_SPLAT_FOV == 4
    a = [f for f in _lib.UdSplat._fields_ if f[0] not in ("K", "nK")]
    b = [f for f in _lib.UdSplatCamera._fields_ if f[0] not in ("params", "cos_limit", "model")]
    assert a == b


P = 0x1000                                              # stands for a device pointer: every refusal comes before any HIP call


def test_camera_project_rejects_bad_descriptors_without_a_launch():
    from unidepth_amd import _lib
    lib = _lib.lib

    def rc(**kw):
        base = dict(xyz=P, params=P, uv=P, batch_stride=30, point_stride=3, comp_stride=1, n_points=10, B=2, H=5, W=7, uv_rows=1)
        base.update(kw)
        models = base.pop("models", (1, 6))
        d = _lib.UdCameraProject()
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(models):
            d.model[b] = m
        return lib.ud_camera_project(C.byref(d), None), lib.ud_last_error().decode()

    assert lib.ud_camera_project(None, None) < 0 and "null descriptor" in lib.ud_last_error().decode()
    for kw, word in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"),
                     (dict(n_points=-1), "bad sizes"), (dict(n_points=1 << 31), "bad sizes"),
                     (dict(xyz=None), "null pointer"), (dict(params=None), "null pointer"), (dict(uv=None), "null pointer"),
                     (dict(point_stride=0), "bad strides"), (dict(comp_stride=0), "bad strides"), (dict(batch_stride=-1), "bad strides"),
                     (dict(uv=P + 4), "8-byte aligned"),
                     (dict(models=(1, 0)), "model tag"), (dict(models=(7, 1)), "model tag"),
                     (dict(T=P, nT=0), "nT"), (dict(T=P, nT=3), "nT")):
        r, msg = rc(**kw)
        assert r < 0 and word in msg and msg.startswith("ud_camera_project:"), (kw, r, msg)
    r, msg = rc(n_points=0)                             # nothing to do: no launch either
    assert r == 0


def test_splat_camera_rejects_bad_descriptors_without_a_launch():
    from unidepth_amd import _lib
    lib = _lib.lib
    B, H, W = 2, 5, 7
    nbytes = lib.ud_splat_work_bytes(B, H, W)

    def rc(**kw):
        base = dict(xyz=P, params=P, depth=P, work=P, work_bytes=nbytes, batch_stride=30, point_stride=3, comp_stride=1, n_points=10,
                    B=B, H=H, W=W, mode=_lib.UD_SPLAT_NEAREST)
        base.update(kw)
        models = base.pop("models", (3, 5))
        d = _lib.UdSplatCamera()
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(models):
            d.model[b] = m
        return lib.ud_splat_camera(C.byref(d), None), lib.ud_last_error().decode()

    assert lib.ud_splat_camera(None, None) < 0 and "null descriptor" in lib.ud_last_error().decode()
    MEAN = _lib.UD_SPLAT_MEAN
    for kw, word in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1, work_bytes=1 << 40), "bad sizes"), (dict(H=0), "bad sizes"),
                     (dict(W=-1), "bad sizes"), (dict(H=65536, W=65536, work_bytes=1 << 60), "bad sizes"),
                     (dict(n_points=-1), "bad sizes"), (dict(n_points=1 << 31), "bad sizes"),
                     (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(flags=8), "unknown flag"),
                     (dict(xyz=None), "null pointer"), (dict(depth=None), "null pointer"),
                     (dict(point_stride=0), "bad strides"), (dict(comp_stride=0), "bad strides"), (dict(batch_stride=-1), "bad strides"),
                     (dict(params=None), "params [B,16]"), (dict(models=(1, 0)), "model tag"), (dict(models=(9, 1)), "model tag"),
                     (dict(T=P, nT=0), "nT"), (dict(T=P, nT=3), "nT"),
                     (dict(color=P), "color and rgb"), (dict(rgb=P), "color and rgb"),
                     (dict(mode=MEAN, index=P), "UD_SPLAT_NEAREST only"), (dict(mode=MEAN, color=P, rgb=P), "UD_SPLAT_NEAREST only"),
                     (dict(work=None), "work is null"), (dict(work=P + 4), "work is null"),
                     (dict(work_bytes=B * H * W * 8 - 1), "work is null"),
                     (dict(work_bytes=B * H * W * 12 - 1, count=P), "work is null"),
                     (dict(work_bytes=B * H * W * 12 - 1, mode=MEAN), "work is null")):
        r, msg = rc(**kw)
        assert r < 0 and word in msg and msg.startswith("ud_splat_camera:"), (kw, r, msg)
    # ud_splat keeps refusing the camera-only flag
    d = _lib.UdSplat()
    for k, v in dict(xyz=P, K=P, depth=P, work=P, work_bytes=nbytes, batch_stride=30, point_stride=3, comp_stride=1, n_points=10, B=B, H=H, W=W,
                     nK=1, flags=_lib.UD_SPLAT_FOV).items():
        setattr(d, k, v)
    assert lib.ud_splat(C.byref(d), None) < 0 and "ud_splat: unknown flag" in lib.ud_last_error().decode()


# ---- argument errors of the Python surface (CPU tensors: every check comes before any launch) -------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, gtpoints, project_camera, render_depth_camera
    from unidepth_amd import reproject as module
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    pts, rows = torch.zeros(2, 3, 6, 8), torch.zeros(2, 50, 3)
    eucm = cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))
    for bad in (dict(points=torch.zeros(2, 4, 6, 8)), dict(points=torch.zeros(2, 50, 2)), dict(points=torch.zeros(50, 3)), dict(points=pts.double()),
                dict(points=[[0.0, 0.0, 1.0]]), dict(points=rows), dict(points=rows, image_shape=(0, 8)), dict(points=pts, image_shape=5),
                dict(points=pts), dict(points=rows, image_shape=(6, 8))):                    # the last two: CPU tensors
        with pytest.raises(ValueError):
            project_camera(bad.pop("points"), eucm, **bad)
    for bad in (dict(points=torch.zeros(2, 4, 6, 8)), dict(points=pts.double()), dict(points=pts, image_shape=(6,)), dict(points=pts, mode="max"),
                dict(points=pts, rounding="round"), dict(points=pts), dict(points=rows)):
        kw = dict(dict(image_shape=(6, 8)), **bad)
        with pytest.raises(ValueError):
            render_depth_camera(kw.pop("points"), eucm, kw.pop("image_shape"), **kw)
    with pytest.raises(ValueError, match="max_angle"):
        render_depth_camera(pts, eucm, (6, 8), max_angle="wide")
    # batch-size mismatches are found by prepare_camera, which needs a device: checked on a prepared camera of the wrong length
    prepared = gtpoints.PreparedCamera(torch.zeros(3, 16), (1, 1, 1))
    with pytest.raises(ValueError):
        gtpoints.prepare_camera(prepared, 2, "cpu")
    for cam in (cameras.Pinhole(K), eucm, cameras.Spherical(torch.tensor([8.0, 11, 26, 18, 53, 37, 3.0, 1.4])),
                cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12)), cameras.Fisheye624(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12)),
                cameras.MEI(torch.tensor([50.0, 51, 26, 18, 0, 0, 0, 0, 1.0])), cameras.BatchCamera([cameras.Pinhole(K), eucm])):
        assert cam.get_projection_mask() is None
        with pytest.raises(RuntimeError, match="GPU"):
            cam.project(pts)
        with pytest.raises(ValueError):
            cam.project(rows)
        assert cam.get_projection_mask() is None
    for name in ("render_depth_camera", "project_camera"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(module, name)
