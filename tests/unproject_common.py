"""What the unproject tests share (not a test module): the cases and numpy restatements of tools/make_golden_unproject.py, each case's
inputs and restatements computed once per process, and the measured bars of tests/golden/unproject.npz."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_unproject", os.path.join(ROOT, "tools", "make_golden_unproject.py"))
up = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(up)
gp, cp = up.gp, up.cp

FORMS = ("raw", "normalize", "depth")
_CACHE = {}


def shape(name):
    return gp.CASES[up.base_case(name)][:2]


def case(name):
    """inputs, the fp32 restatement of every form, the fp64 restatement of the raw form and the solver record, computed once and shared"""
    if name not in _CACHE:
        uv, depth, params, models = up.case_inputs(name)
        info = {}
        raw, mask = up.unproject(uv, params, models, np.float32, info)
        r64, m64 = up.unproject(uv, params, models, np.float64)
        nrm = up.unproject(uv, params, models, np.float32, normalize=True)[0]
        dep = up.unproject(uv, params, models, np.float32, depth=depth)[0]
        _CACHE[name] = dict(uv=uv, depth=depth, params=params, models=models, raw=raw, normalize=nrm, mask=mask, r64=r64, m64=m64, info=info)
        _CACHE[name]["depth_form"] = dep
    return _CACHE[name]


def form(c, which):
    return c["depth_form" if which == "depth" else which]


def golden():
    if "golden" not in _CACHE:
        _CACHE["golden"] = dict(np.load(up.GOLDEN))
    return _CACHE["golden"]


def bars():
    return {m: up.bar(float(golden()["referr." + n])) for m, n in up.MODEL_NAMES.items()}


def same_specials(a, b):
    """NaN, +inf and -inf in the same places"""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


def same_bits(a, b):
    """bit for bit, the sign of a zero included; a NaN equals a NaN whatever its sign and payload"""
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def assert_within_bars(out, ref, truth, models, bars, what):
    """rays [B,N,3]: NaN exactly where the truth has NaN, |out - ref| / max(|truth|, 1e-4) within the bar of the image's model on every
    point.  Returns the worst ratio to the bar."""
    assert np.array_equal(np.isnan(out), np.isnan(truth)), f"{what}: NaN positions differ"
    with np.errstate(invalid="ignore"):
        e = up.ray_error(np.where(np.isnan(truth), 0.0, out.astype(np.float64) - ref.astype(np.float64)), truth)
    worst = 0.0
    for b, m in enumerate(models):
        eb = float(e[b].max())
        assert eb <= bars[m], f"{what}: image {b} ({up.MODEL_NAMES[m]}) error {eb:.3e} above the bar {bars[m]:.3e}"
        worst = max(worst, eb / bars[m])
    return worst
