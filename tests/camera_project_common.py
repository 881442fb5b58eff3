"""What the camera-projection tests share (not a test module): the cases and numpy restatements of tools/make_golden_camera_project.py,
each case's inputs and restatements computed once per process, the measured bars of tests/golden/camera_project.npz and the every-point
comparison."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_camera_project", os.path.join(ROOT, "tools", "make_golden_camera_project.py"))
cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cp)
gp = cp.gp

EXACT = (cp.PINHOLE, cp.EUCM, cp.OPENCV, cp.MEI)             # no libm function beyond sqrt: bit-equal to the fp32 restatement
_CACHE = {}
_GOLDEN = {}


def golden():
    if not _GOLDEN:
        _GOLDEN.update(np.load(cp.GOLDEN))
    return _GOLDEN


def case(name):
    """inputs and both restatements of a case, computed once and shared (never modified)"""
    if name not in _CACHE:
        xyz, params, models, n_reg = cp.case_inputs(name)
        H, W = gp.CASES[name][:2]
        uv32, in32, d32 = cp.project(xyz, params, models, (H, W), None, np.float32)
        uv64, in64, d64 = cp.project(xyz, params, models, (H, W), None, np.float64)
        _CACHE[name] = dict(xyz=xyz, params=params, models=models, n_reg=n_reg, H=H, W=W, uv32=uv32, in32=in32, d32=d32, uv64=uv64, in64=in64)
    return _CACHE[name]


def bars():
    g = golden()
    return {m: cp.bar(float(g["referr." + n])) for m, n in cp.MODEL_NAMES.items()}


def same_bits(a, b):
    """equal bit for bit, any NaN standing for any other NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def assert_uv(out, c, bars, what, ref=None):
    """out [B,N,2] against the fp32 restatement on EVERY point: NaN and infinities in the same places with the same sign; bit-equal for
    the models without a libm function, |out - r32| / max(|truth|, 1) within the model's bar for Spherical and Fisheye624.  With ref
    (the reference's uv [B,N,2]): additionally within the bar of it on the regular points.  Returns the worst ratio to the bar."""
    worst = 0.0
    for b, m in enumerate(c["models"]):
        o, r = out[b], c["uv32"][b]
        assert np.array_equal(np.isnan(o), np.isnan(r)), f"{what}: image {b}: NaN positions differ"
        inf = np.isinf(r)
        assert np.array_equal(o[inf], r[inf]) and np.array_equal(np.isinf(o), inf), f"{what}: image {b}: infinities differ"
        if m in EXACT:
            assert same_bits(o, r), f"{what}: image {b} ({cp.MODEL_NAMES[m]}) is not bit-equal to the fp32 restatement"
        else:
            fin = np.isfinite(r)
            e = cp.uv_error(np.where(fin, o, 0).astype(np.float64) - np.where(fin, r, 0), np.where(fin, c["uv64"][b], 0))
            assert e.max() <= bars[m], f"{what}: image {b} ({cp.MODEL_NAMES[m]}) {e.max():.3e} from the restatement, bar {bars[m]:.3e}"
            worst = max(worst, float(e.max()) / bars[m])
        if ref is not None:
            reg = slice(0, c["n_reg"])
            e = cp.uv_error(o[reg].astype(np.float64) - ref[b][reg], c["uv64"][b][reg])
            assert e.max() <= bars[m], f"{what}: image {b} ({cp.MODEL_NAMES[m]}) {e.max():.3e} from the reference, bar {bars[m]:.3e}"
            worst = max(worst, float(e.max()) / bars[m])
    return worst


def rows_of(planar):
    """[B,C,H,W] -> [B,N,C]"""
    B, C = planar.shape[:2]
    return np.ascontiguousarray(planar.reshape(B, C, -1).transpose(0, 2, 1))
