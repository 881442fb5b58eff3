"""gt_points without a GPU (unidepth_amd/gtpoints.py, include/unidepth_hip.h UdReconstruct): the numpy fp32 restatement of
tools/make_golden_gt_points.py against the reference's own Camera.reconstruct arrays (tests/golden/gt_points.npz) at the measured bar,
the conditions the generator promises (residual maxima outside [0.5e-3, 2e-3], the paths the cases must reach), the NOT normalised
functions of csrc/camera_models.h compiled for the host (tests/recon_host/recon_host.cpp, a stand-alone program), the Python argument
errors and the C-ABI's workspace query and argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gt_points_common as common
import host_program

ROOT = common.ROOT
gp = common.gp
_case, _bars, assert_within_bars = common.case, common.bars, common.assert_within_bars


def test_golden_has_every_case():
    g = np.load(gp.GOLDEN)
    want = [f"{n}.{k}" for n in gp.CASES for k in ("depth", "params", "models", "out", "steps")] + ["referr." + n for n in gp.MODEL_NAMES.values()]
    assert sorted(g.files) == sorted(want)
    for name, (H, W, cams, B) in gp.CASES.items():
        depth, params, models = gp.case_rows(name)
        assert g[name + ".out"].dtype == np.float32 and g[name + ".out"].shape == (B, 3, H, W)
        # the seeded inputs are the stored ones, bit for bit (NaN included)
        assert np.array_equal(g[name + ".depth"].view(np.uint32), depth.view(np.uint32)) and depth.shape == (B, 1, H, W)
        assert np.array_equal(g[name + ".params"], params) and list(g[name + ".models"]) == models
    assert os.path.getsize(gp.GOLDEN) < 1024 * 1024
    assert {(5, 7), (9, 29), (37, 53)} == {c[:2] for c in gp.CASES.values()}
    for m in gp.MODEL_NAMES:                                  # one case per model at B = 2 with different parameters per image
        assert any(B == 2 and [c[0] for c in cams] == [m, m] and cams[0][1] != cams[1][1] for _, _, cams, B in gp.CASES.values()), m
    assert sorted(c[0] for c in gp.CASES["mixed_5x7_b6"][2]) == sorted(gp.MODEL_NAMES)
    assert len(gp.CASES["broadcast_opencv_9x29_b3"][2]) == 1 and gp.CASES["broadcast_opencv_9x29_b3"][3] == 3


def test_cases_reach_the_paths_they_are_there_for():
    f32 = np.float32
    # depths: 0, negatives, below 1e-4, one NaN per case
    for name in gp.CASES:
        d = gp.case_inputs(name)[0]
        assert (d == 0).any() and (d < 0).any() and ((d > 0) & (d < 1e-4)).any() and np.isnan(d).sum() == 1
    # OPENCV: radial only / tangential + thin prism without radial / every term
    def flags(row):
        return (np.abs(row[4:10]).sum() > 1e-6, np.abs(row[10:12]).sum() > 1e-6, np.abs(row[12:16]).sum() > 1e-6)
    seen = set()
    for name in gp.CASES:
        _, params, models = gp.case_inputs(name)
        seen |= {flags(r) for r, m in zip(params, models) if m == gp.OPENCV}
        for r, m in zip(params, models):
            if m == gp.OPENCV:
                assert np.abs(r[7:10]).sum() == 0
    assert {(True, False, False), (False, True, True), (True, True, True)} <= seen
    assert any((np.abs(r[7:10]) > 0).all() for r, m in zip(*gp.case_inputs("fisheye624_9x29_b2")[1:]) if m == gp.FISHEYE624)
    _, p, _ = gp.case_inputs("mei_37x53_b2")
    assert p[0, 8] == f32(1.0) and p[1, 8] != f32(1.0)
    c = _case("mei_37x53_b2")
    H, W = c["depth"].shape[-2:]
    uf, vf = np.meshgrid(np.arange(W, dtype=f32) + f32(0.5), np.arange(H, dtype=f32) + f32(0.5))
    with np.errstate(all="ignore"):
        pz = gp._mei(c["params"][1], uf, vf, f32)[2]
    assert (pz < 1e-4).sum() > 50 and (pz > 1e-4).sum() > 50, "the wide MEI camera must have pixels on both sides of the z floor"
    _, p, _ = gp.case_inputs("eucm_9x29_b2")
    assert p[0, 4] < 0.5 < p[1, 4]
    _, p, _ = gp.case_inputs("spherical_37x53_b2")
    assert (p[1, 4], p[1, 5]) != (53.0, 37.0)                 # a crop: the panorama's size is not the image's
    # the OPENCV pair that needs different iteration counts
    st = _case("opencv_37x53_b2_iters")["info"]["steps"]
    assert 1 <= st[0] <= 2 < st[1]


def test_residual_maxima_keep_clear_of_the_exit_threshold():
    """every OPENCV / Fisheye624 camera of every case, every iteration: the fp32 restatement's image-wide max |residual| lies outside
    [0.5e-3, 2e-3], so a library whose last bit differs cannot flip the early exit; the iteration counts are the reference's"""
    g = np.load(gp.GOLDEN)
    n = 0
    for name in gp.CASES:
        c = _case(name)
        for b, m in enumerate(c["models"]):
            if m in gp.ITERATIVE:
                maxima = c["info"].get("maxima", {}).get(b, [])
                assert gp.margins_ok(maxima), (name, b, maxima)
                assert c["info"].get("steps", {}).get(b, 0) == int(g[name + ".steps"][b]), (name, b)
                n += 1
            else:
                assert int(g[name + ".steps"][b]) == -1
    assert n >= 12


@pytest.mark.parametrize("name", list(gp.CASES))
def test_fp32_restatement_within_measured_bar_of_reference(name):
    c = _case(name)
    ref = np.load(gp.GOLDEN)[name + ".out"]
    assert np.array_equal(np.isnan(ref), np.isnan(c["r64"]))
    w = assert_within_bars(c["r32"], ref, c, _bars(), name)
    print(f"{name}: fp32 restatement uses {w:.3f} of the bar")


def test_bars_come_from_the_reference_error():
    g = np.load(gp.GOLDEN)
    for m, n in gp.MODEL_NAMES.items():
        e = float(g["referr." + n])
        assert 0 < e < 1e-2 and gp.bar(e) == max(4 * e, 8 * 2.0 ** -24)
    # the stored maxima are what the stored outputs give against the fp64 restatement
    worst = {}
    for name in gp.CASES:
        c = _case(name)
        e = gp.error_ratio(g[name + ".out"].astype(np.float64) - c["r64"], c["r64"], c["depth"])
        for b, m in enumerate(c["models"]):
            worst[m] = max(worst.get(m, 0.0), float(e[b].max()))
    for m, n in gp.MODEL_NAMES.items():
        assert abs(worst[m] - float(g["referr." + n])) <= 1e-6 * worst[m], n      # the fp64 restatement's libm may differ in its last bit


# ---- the NOT normalised header functions, compiled for the host ------------------------------------------------------------------

@pytest.fixture(scope="module")
def recon_host(tmp_path_factory):
    out = host_program.build(tmp_path_factory, "recon_host", sanitize=False)

    def run(model, H, W, row):
        steps, blocks = host_program.run(out, [model, H, W] + [float(v).hex() for v in row], [], [4, 4 * 9 * H * W])
        steps = int(np.frombuffer(steps, dtype=np.int32)[0])
        blocks = np.frombuffer(blocks, dtype=np.float32).reshape(3, 3, H, W)
        return steps, blocks[0], blocks[1], blocks[2]
    return run


def _host_cameras():
    for name in gp.CASES:
        H, W = gp.CASES[name][:2]
        _, params, models = gp.case_inputs(name)
        for i, (row, m) in enumerate(zip(params, models)):
            if m in (gp.OPENCV, gp.FISHEYE624, gp.MEI):
                yield pytest.param(name, i, id=f"{name}-{i}")


@pytest.mark.parametrize("name,i", list(_host_cameras()))
def test_unnormalised_header_functions_on_the_host(recon_host, name, i):
    """ud_cam_finish_radial_dir / ud_cam_mei_dir over the cases: equal to the fp32 restatement (bit for bit where no libm function is
    involved; Fisheye624's tanf within 4 units in the last place), same iteration count, and normalising them reproduces the existing
    normalised functions bit for bit"""
    f32 = np.float32
    H, W = gp.CASES[name][:2]
    _, params, models = gp.case_inputs(name)
    row, m = params[i], models[i]
    steps, raw, nrm, old = recon_host(m, H, W, row)
    assert np.array_equal(nrm.view(np.uint32), old.view(np.uint32)), "normalising the new functions must reproduce the old ones bitwise"
    uf, vf = np.meshgrid(np.arange(W, dtype=f32) + f32(0.5), np.arange(H, dtype=f32) + f32(0.5))
    with np.errstate(all="ignore"):
        if m == gp.MEI:
            want = np.stack(gp._mei(row, uf, vf, f32))
        else:
            dx, dy, _, st = gp._solve_radial(row, m, uf, vf, f32)
            want = np.stack([dx, dy, np.ones_like(dx)])
            assert steps == st
    assert want.dtype == np.float32 and np.isfinite(raw).all()
    if m == gp.FISHEYE624:
        assert (np.abs(raw - want) <= 4 * np.spacing(np.abs(want))).all()
    else:
        assert np.array_equal(raw.view(np.uint32), want.view(np.uint32))


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    from unidepth_amd import _lib, cameras, gtpoints
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    d = torch.ones(2, 1, 5, 7)
    for bad in (torch.ones(5, 7), torch.ones(2, 2, 5, 7), torch.ones(1, 2, 1, 5, 7), torch.ones(2, 1, 5, 7, dtype=torch.int32),
                torch.ones(0, 1, 5, 7), torch.ones(2, 1, 0, 7)):
        with pytest.raises(ValueError):
            gtpoints.gt_points(bad, K)
    for bad_cam in (K.expand(3, 3, 3), torch.ones(2, 4), torch.ones(3, 3, dtype=torch.int64), cameras.Pinhole(K.expand(3, 3, 3)),
                    cameras.EUCM(torch.tensor([[50.0, 51, 26, 18, 0.5, 1.0]] * 3)),
                    cameras.BatchCamera([cameras.Pinhole(K)] * 3), cameras.BatchCamera([cameras.MEI(torch.tensor([50.0, 51, 26, 18, 0, 0, 0, 0, 1.0]))])):
        with pytest.raises(ValueError):
            gtpoints.gt_points(d, bad_cam)
    skew = K.clone()
    skew[0, 1] = 0.25
    with pytest.raises(ValueError, match="skew"):
        gtpoints.gt_points(d, skew)
    with pytest.raises(ValueError, match=str(_lib.UD_RECON_MAX_B)):
        gtpoints.gt_points(torch.ones(_lib.UD_RECON_MAX_B + 1, 1, 1, 1), K)
    # well-formed arguments on the CPU: the HIP kernels are the only implementation
    for cam in (K, cameras.Pinhole(K), cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12)),
                cameras.BatchCamera([cameras.Pinhole(K), cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))])):
        with pytest.raises(RuntimeError, match="GPU"):
            gtpoints.gt_points(d, cam)
        with pytest.raises(RuntimeError, match="GPU"):
            gtpoints.gt_points(d[:, 0], cam)
    with pytest.raises(RuntimeError, match="GPU"):
        cameras.Pinhole(K).reconstruct(d)
    with pytest.raises(RuntimeError, match="GPU"):
        gtpoints.add_points({"depth": d, "camera": K})
    with pytest.raises(NotImplementedError):
        gtpoints.gt_points(d, object())
    for cls in (cameras.Pinhole, cameras.EUCM, cameras.Spherical, cameras.OPENCV, cameras.Fisheye624, cameras.MEI, cameras.BatchCamera):
        assert callable(cls.reconstruct)
    import unidepth_amd
    for name in ("gt_points", "add_points", "prepare_camera"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(gtpoints, name)
    from unidepth_amd import eval_ops
    assert callable(eval_ops.MetricsAccumulator.accumulate_metrics)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_work_bytes_and_c_abi_argument_checks():
    from unidepth_amd import _lib
    wb = _lib.lib.ud_reconstruct_work_bytes
    assert wb(2, 5, 7, 0) == 0
    assert wb(2, 5, 7, 1) == 48 + 35 * 16 and wb(6, 37, 53, 2) == 96 + 2 * 37 * 53 * 16      # 11 maxima per image rounded up to 16 bytes + float4 states
    assert wb(8, 480, 640, 8) % 16 == 0
    for bad in ((0, 4, 4, 0), (1, 0, 4, 0), (1, 4, 0, 0), (_lib.UD_RECON_MAX_B + 1, 4, 4, 0), (2, 4, 4, 3), (2, 4, 4, -1), (1, 65536, 32768, 0)):
        assert wb(*bad) == -1, bad
    lib = _lib.lib
    assert lib.ud_reconstruct(None, None) < 0 and "null descriptor" in lib.ud_last_error().decode()

    def call(**kw):
        d = _lib.UdReconstruct()
        base = dict(depth=16, params=16, points=16, work=16, work_bytes=1 << 20, B=2, H=5, W=7)
        base.update(kw)
        models = base.pop("models", (1, 4))
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(models):
            d.model[b] = m
        return lib.ud_reconstruct(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(depth=None), "null pointer"),
                    (dict(params=None), "null pointer"), (dict(points=None), "null pointer"), (dict(work=None), "null pointer"),
                    (dict(work=24), "16-byte aligned"), (dict(work_bytes=48 + 35 * 16 - 1), "smaller than"),
                    (dict(models=(1, 0)), "model tag"), (dict(models=(7, 1)), "model tag")):
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
