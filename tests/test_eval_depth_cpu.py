"""The 2-D depth metrics' golden file (tests/golden/eval_depth.npz, written by tools/make_golden_eval_depth.py from the reference's own
eval_depth on the CPU) and the numpy restatement of the definitions that the GPU tests use at sizes too large for a golden file."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_eval_depth", os.path.join(ROOT, "tools", "make_golden_eval_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mg = _tool()


def _golden(name):
    g = np.load(mg.GOLDEN)
    return {k: g[f"{name}.{k}"] for k in mg.KEYS}


def test_golden_has_every_case_and_key_in_reference_order():
    g = np.load(mg.GOLDEN)
    names = list(g.files)
    for case, (B, *_rest) in mg.CASES.items():
        keys = [n.split(".", 1)[1] for n in names if n.split(".", 1)[0] == case]
        assert tuple(keys) == mg.KEYS, case
        for k in keys:
            assert g[f"{case}.{k}"].shape == (B,) and g[f"{case}.{k}"].dtype == np.float32


def test_golden_edge_case_semantics():
    """empty V -> NaN everywhere; p = 0 inside V -> inf / NaN where the definitions give them; two valid pixels -> finite."""
    g = _golden("edge_b3_empty_zero_two")
    assert all(np.isnan(g[k][0]) for k in mg.KEYS)
    assert np.isinf(g["rmselog"][1]) and np.isinf(g["log10"][1]) and np.isnan(g["silog"][1])
    assert all(np.isfinite(g[k][2]) for k in mg.KEYS)


@pytest.mark.parametrize("name", list(mg.CASES))
def test_restatement_matches_reference_golden(name):
    gts, preds, masks, max_depth = mg.case_inputs(name)
    got, ns = mg.restate(gts, preds, masks, max_depth)
    assert mg.compare(got, _golden(name), ns) == []


def test_restatement_resample_is_torch_bilinear():
    """the fp32 resample of the restatement against F.interpolate on the CPU (upsampling and downsampling).  Not bit-exact: an x86
    torch build may contract the source index and the blend into FMAs (a one-ulp change of the source index moves lambda by ~1e-6 at
    these sizes), where the definition -- and the HIP kernel -- round every operation separately."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(7)
    for (h, w), (H, W) in (((37, 53), (120, 160)), ((101, 131), (48, 64)), ((7, 9), (7, 9))):
        x = torch.rand(1, 1, h, w, generator=g) * 10 + 0.1
        ref = F.interpolate(x, size=(H, W), mode="bilinear").numpy()[0, 0]
        got = mg.resample(x.numpy()[0, 0], H, W)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0)


@pytest.mark.skipif(not os.path.isfile(mg.reference_path()), reason="reference tree not present (authoring machine only)")
def test_reference_rerun_reproduces_golden():
    ref = mg.reference_eval_depth()
    for name in mg.CASES:
        vals, order = mg.reference_outputs(ref, name)
        assert tuple(order) == mg.KEYS
        g = _golden(name)
        for k in mg.KEYS:
            np.testing.assert_array_equal(vals[k], g[k], err_msg=f"{name}.{k}")
