"""GPU parity of the 2-D depth metrics (unidepth_amd/eval_ops.py eval_depth / DICT_METRICS -> ud_eval_depth, csrc/evaldepth.hip) against
the reference's own eval_depth (tests/golden/eval_depth.npz) and, at the sizes users run, against the numpy restatement of the
definitions in tools/make_golden_eval_depth.py (pinned to the golden file by tests/test_eval_depth_cpu.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_eval_depth", os.path.join(ROOT, "tools", "make_golden_eval_depth.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


def _run(gts, preds, masks, max_depth=None):
    from unidepth_amd import eval_ops
    res = eval_ops.eval_depth(gts.cuda(), preds.cuda(), masks.cuda(), max_depth=max_depth)
    assert tuple(res) == mg.KEYS
    for v in res.values():
        assert v.is_cuda and v.dtype == torch.float32 and v.shape == (gts.shape[0],)
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", list(mg.CASES))
def test_eval_depth_matches_reference_golden(name):
    gts, preds, masks, max_depth = mg.case_inputs(name)
    g = np.load(mg.GOLDEN)
    ref = {k: g[f"{name}.{k}"] for k in mg.KEYS}
    _, ns = mg.restate(gts, preds, masks, max_depth)
    got = _run(gts, preds, masks, max_depth)
    assert mg.compare(got, ref, ns) == []


@pytest.mark.parametrize("B,HW,hw,kind", [(8, (480, 640), (480, 640), "dense"), (4, (375, 1242), (266, 882), "sparse"),
                                          (1, (1080, 1920), (1080, 1920), "dense")])
def test_eval_depth_matches_restatement_at_user_sizes(B, HW, hw, kind):
    g = torch.Generator().manual_seed(B * 7919 + HW[0])
    gts, preds, masks = mg.random_inputs(g, B, HW, hw, kind)
    if kind == "dense":
        masks[:] = True
    ref, ns = mg.restate(gts, preds, masks)
    got = _run(gts, preds, masks)
    assert mg.compare(got, ref, ns) == []


def test_dict_metrics_equal_eval_depth_on_one_image():
    from unidepth_amd import eval_ops
    gts, preds, masks, _ = mg.case_inputs("equal_b2_60x80")
    m = masks[0, 0]
    gt, pred = gts[0, 0][m].cuda(), preds[0, 0][m].cuda()
    n = gt.shape[0]
    res = eval_ops.eval_depth(gt.view(1, 1, 1, n), pred.view(1, 1, 1, n), torch.ones(1, 1, 1, n, dtype=torch.bool, device="cuda"))
    assert set(eval_ops.DICT_METRICS) == {k for k in mg.KEYS if not k.endswith(("_ssi", "_si"))}
    for name, fn in eval_ops.DICT_METRICS.items():
        v = fn(gt, pred)
        assert v.ndim == 0 and v.is_cuda
        assert v.view(1).view(torch.int32).item() == res[name].view(torch.int32).item(), name
    a1 = eval_ops.DICT_METRICS_D["a1"](gt, pred)
    ar = eval_ops.DICT_METRICS_D["abs_rel"](gt, pred)
    assert a1.shape == gt.shape and a1.dtype == torch.float32 and ar.shape == gt.shape
    assert abs(float(1.0 - a1.mean()) - float(res["d1"][0])) * n <= 1.0 + 1e-3      # d1 counts r < 1.25, a1 marks r > 1.25


def test_eval_depth_bitwise_reproducible():
    g = torch.Generator().manual_seed(5)
    gts, preds, masks = mg.random_inputs(g, 4, (375, 1242), (266, 882), "sparse")
    a = _run(gts, preds, masks, 30.0)
    b = _run(gts, preds, masks, 30.0)
    for k in mg.KEYS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_eval_depth_no_host_sync():
    from unidepth_amd import eval_ops
    g = torch.Generator().manual_seed(6)
    gts, preds, masks = (t.cuda() for t in mg.random_inputs(g, 2, (120, 160), (37, 53), "dense"))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = eval_ops.eval_depth(gts, preds, masks, max_depth=12.0)
        res = eval_ops.eval_depth(gts, preds.half(), masks, max_depth=None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(res["d1"]).all()


def test_eval_depth_argument_errors():
    from unidepth_amd import eval_ops
    gt = torch.rand(2, 1, 8, 8, device="cuda") + 1
    m = torch.ones(2, 1, 8, 8, dtype=torch.bool, device="cuda")
    with pytest.raises(ValueError):
        eval_ops.eval_depth(torch.rand(2, 2, 8, 8, device="cuda"), gt, m)
    with pytest.raises(ValueError):
        eval_ops.eval_depth(gt, gt[:1], m)
    with pytest.raises(ValueError):
        eval_ops.eval_depth(gt, gt, m[:1])
    with pytest.raises(ValueError):
        eval_ops.eval_depth(gt[:0], gt[:0], m[:0])
