"""What the gt_points tests share (not a test module): the cases and numpy restatements of tools/make_golden_gt_points.py, each case's
inputs and restatements computed once per process, the measured bars of tests/golden/gt_points.npz and the every-pixel comparison."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_gt_points", os.path.join(ROOT, "tools", "make_golden_gt_points.py"))
gp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gp)

_CACHE = {}


def case(name):
    """inputs, both restatements and the solver record of a case, computed once and shared"""
    if name not in _CACHE:
        depth, params, models = gp.case_rows(name)
        info = {}
        r32 = gp.restate(depth, params, models, np.float32, info)
        r64 = gp.restate(depth, params, models, np.float64)
        _CACHE[name] = dict(depth=depth, params=params, models=models, r32=r32, r64=r64, info=info)
    return _CACHE[name]


def bars():
    g = np.load(gp.GOLDEN)
    return {m: gp.bar(float(g["referr." + n])) for m, n in gp.MODEL_NAMES.items()}


def assert_within_bars(out, ref, case, bars, what):
    """every point of every image: NaN exactly where the fp64 restatement has NaN, |out - ref| / max(|truth|, 1e-4 max(|depth|, 1))
    within the bar of the image's model.  Returns the worst ratio to the bar."""
    truth = case["r64"]
    assert np.array_equal(np.isnan(out), np.isnan(truth)), f"{what}: NaN positions differ"
    e = gp.error_ratio(out.astype(np.float64) - ref.astype(np.float64), truth, case["depth"])
    worst = 0.0
    for b, m in enumerate(case["models"]):
        eb = float(e[b].max())
        assert eb <= bars[m], f"{what}: image {b} ({gp.MODEL_NAMES[m]}) error {eb:.3e} above the bar {bars[m]:.3e}"
        worst = max(worst, eb / bars[m])
    return worst
