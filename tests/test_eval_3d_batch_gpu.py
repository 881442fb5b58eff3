"""GPU parity of eval_3d_batch (unidepth_amd/eval_ops.py -> ud_eval_3d, csrc/eval3d.hip) against the reference's own eval_3d
(tests/golden/eval_3d_batch.npz, and the two eval3d cases of tests/golden/eval_knn.npz) and against the numpy restatement of
tests/eval3d_restate.py (pinned to the golden file by tests/test_eval_3d_batch_cpu.py); empty images, determinism, guarded outputs,
input layouts, no host synchronisation, and MetricsAccumulator.

Every case runs once per process (_gpu_case) and is shared.  The restatement's brute-force numpy search takes a minute on the three
large cases, so there its distances come from ud_knn_points (eval_ops.knn_points, pinned bit-exact to the numpy search by
tests/test_eval_ops_gpu.py); size, sampling, compaction, counts, sums and F1 stay numpy.  The small cases use the numpy search."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import eval3d_restate as er
import layout_guard as lg
from oracle import make_golden_eval as mge

pytestmark = pytest.mark.gpu

LARGE = ("edge_b8_100", "full_518_b3", "quarter_518_b3")
KNN_GOLDEN = tuple(f"eval3d.{n}" for n in mge.EVAL3D_CASES)         # the cases already stored in tests/golden/eval_knn.npz


def _inputs(name):
    if name.startswith("eval3d."):
        return mge.eval3d_case_inputs(name.split(".", 1)[1])
    return er.case_inputs(name)


def _to_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _run(gts, preds, masks, th):
    from unidepth_amd import eval_ops
    B = gts.shape[0]
    res = eval_ops.eval_3d_batch(gts.cuda(), preds.cuda(), masks.cuda(), th.cuda() if isinstance(th, torch.Tensor) else th)
    assert tuple(res) == er.KEYS + ("count", "size")
    for k in er.KEYS:
        assert res[k].is_cuda and res[k].dtype == torch.float32 and res[k].shape == (B,)
    assert res["count"].is_cuda and res["count"].dtype == torch.int64 and res["count"].shape == (B,)
    assert res["size"].is_cuda and res["size"].dtype == torch.int32 and res["size"].shape == (2,)
    return _to_numpy(res)


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    return _run(*_inputs(name))


def _gpu_knn(p1, p2):
    from unidepth_amd import eval_ops
    r = eval_ops.knn_points(torch.from_numpy(p1)[None].cuda(), torch.from_numpy(p2)[None].cuda(), K=1)
    return r.dists[0, :, 0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _restated(name):
    if name in LARGE or name == "eval3d.resampled":
        return er.restate(*_inputs(name), knn=_gpu_knn)
    return er.restate(*_inputs(name))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", er.CASES + KNN_GOLDEN)
def test_matches_reference_golden(golden_dir, name):
    """out[name][count > 0] is what the reference's eval_3d returns (it skips empty images)"""
    got = _gpu_case(name)
    if name.startswith("eval3d."):
        g = np.load(f"{golden_dir}/eval_knn.npz")
        ref = {k: g[f"{name}.{k}"] for k in er.KEYS}
    else:
        ref = er.golden(name)
    keep = got["count"] > 0
    for k in er.KEYS:
        print(name, k, got[k][keep], ref[k])
        np.testing.assert_allclose(got[k][keep], ref[k], rtol=er.RTOL, atol=0, err_msg=f"{name}.{k}")


@pytest.mark.parametrize("name", er.CASES + KNN_GOLDEN)
def test_matches_restatement(name):
    got, ref = _gpu_case(name), _restated(name)
    assert tuple(got["size"]) == ref["size"]
    np.testing.assert_array_equal(got["count"], ref["count"])
    for k in er.KEYS:
        print(name, k, got[k], ref[k])
        np.testing.assert_allclose(got[k], ref[k], rtol=er.RTOL, atol=0, equal_nan=True, err_msg=f"{name}.{k}")


def test_matches_restatement_over_more_than_256_tiles():
    """263 tiles per image: e3_scan_kernel sweeps a second chunk with the carry of the first.  No resampling (518 x 518, about 3,000
    valid pixels per image), valid pixels in the tiles 0, 255, 256 and the partial last one, an empty tile 1 in one image
    (eval3d_restate.many_tiles_inputs asserts all that on the host); the assertions of test_matches_restatement"""
    inputs = er.many_tiles_inputs()
    got, ref = _run(*inputs), er.restate(*inputs)
    assert tuple(got["size"]) == ref["size"] == er.MANY_TILES_HW
    np.testing.assert_array_equal(got["count"], ref["count"])
    for k in er.KEYS:
        print("many_tiles", k, got[k], ref[k])
        np.testing.assert_allclose(got[k], ref[k], rtol=er.RTOL, atol=0, equal_nan=True, err_msg=f"many_tiles.{k}")


def test_ties_lattice_reproduces_f1_of_the_integer_counts():
    """squared distances equal to a threshold (1, 2, 4 on an integer lattice) are NOT counted: F1 is bit for bit the value of the
    restatement's integer counts under strict <"""
    got, ref = _gpu_case("ties_lattice"), er.restated_case("ties_lattice")
    for b, n in enumerate(ref["count"]):
        want = er.f1_from_counts(ref["c1"][b], ref["c2"][b], int(n))
        assert _bits(got["F1"][b:b + 1])[0] == _bits(np.array([want], np.float32))[0], (b, got["F1"][b], want)


def test_empty_images_give_nan_and_zero_count():
    got = _gpu_case("empty_middle")
    assert got["count"][1] == 0 and got["count"][2] == 1 and got["count"][0] > 1
    for k in er.KEYS:
        assert np.isnan(got[k][1]) and np.isfinite(got[k][[0, 2]]).all(), k
    gts, preds, masks, th = er.case_inputs("empty_middle")
    none = _run(gts, preds, torch.zeros_like(masks), th)              # S = 0: every image is empty, the size is the input's
    assert none["count"].tolist() == [0, 0, 0] and tuple(none["size"]) == (37, 53)
    assert all(np.isnan(none[k]).all() for k in er.KEYS)
    one = _run(gts[2:], preds[2:], masks[2:], th)                     # the single-point cloud alone
    assert one["count"].tolist() == [1]
    for k in er.KEYS:
        assert _bits(one[k])[0] == _bits(got[k][2:3])[0], k


def test_bitwise_reproducible():
    a = _gpu_case("quarter_518_b3")
    b = _run(*er.case_inputs("quarter_518_b3"))
    for k in er.KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["size"], b["size"])


ISENT = 0x5A5A5A5A


def _int_guarded(n, dtype, pad=64):
    buf = torch.full((pad + n + pad,), ISENT, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + n], pad


def _int_guard_intact(buf, n, pad):
    return bool((buf[:pad] == ISENT).all()) and bool((buf[pad + n:] == ISENT).all())


@pytest.mark.parametrize("name", ["empty_middle", "eval3d.resampled"])
def test_outputs_and_work_area_stay_inside_their_allocations(name):
    """out, counts, size and the work area sit inside sentinel-filled allocations; the descriptor is driven directly"""
    from unidepth_amd import _lib, eval_ops
    from unidepth_amd.ops import cur_stream, mk
    gts, preds, masks, th = _inputs(name)
    B, _, H, W = gts.shape
    T = len(th)
    gt, pred = gts.cuda().contiguous(), preds.cuda().contiguous()
    mask = masks.cuda().reshape(B, H, W).contiguous().view(torch.uint8)
    thr = torch.tensor(th, dtype=torch.float32, device="cuda")
    nbytes = int(_lib.lib.ud_eval_3d_work_bytes(B, H, W, T))
    cbuf, counts, cpad = _int_guarded(B, torch.int64)
    sbuf, size, spad = _int_guarded(2, torch.int32)
    wpad = 4096
    wbuf = torch.full((wpad + nbytes + wpad,), 0xA5, dtype=torch.uint8, device="cuda")
    # the C-ABI's out is dense [3, B]: one row of 3 * B floats inside a sentinel-filled allocation
    dense = lg.guarded(1, 3 * B, 3 * B + 7, torch.float32, pre_rows=2, post_rows=2, offset_cols=3)
    d = mk(_lib.UdEval3d, gt=gt, pred=pred, mask=mask, thresholds=thr, out=dense.ptr(), counts=counts, size=size,
           work=wbuf[wpad:wpad + nbytes], work_bytes=nbytes, B=B, H=H, W=W, T=T)
    _lib.check(_lib.lib.ud_eval_3d(C.byref(d), cur_stream()), "ud_eval_3d")
    torch.cuda.synchronize()
    dense.check_guards("out")
    assert _int_guard_intact(cbuf, B, cpad), "counts: guard rewritten"
    assert _int_guard_intact(sbuf, 2, spad), "size: guard rewritten"
    assert bool((wbuf[:wpad] == 0xA5).all()) and bool((wbuf[wpad + nbytes:] == 0xA5).all()), "work area: guard rewritten"
    ref = _gpu_case(name)
    got = dense.view.reshape(3, B).cpu().numpy()
    for k, key in enumerate(er.KEYS):
        assert np.array_equal(_bits(got[k]), _bits(ref[key])), key
    assert np.array_equal(counts.cpu().numpy(), ref["count"]) and np.array_equal(size.cpu().numpy(), ref["size"])
    assert eval_ops.EVAL_3D_KEYS == er.KEYS


def test_input_layouts_and_dtypes_give_the_same_result():
    from unidepth_amd import eval_ops
    gts, preds, masks, th = er.case_inputs("empty_middle")
    B, _, H, W = gts.shape
    ref = _gpu_case("empty_middle")
    g_nc = gts.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                  # channels-last memory
    wide = torch.zeros(B, 3, H, W + 9, device="cuda")
    wide[..., 4:4 + W] = preds.cuda()
    p_nc = wide[..., 4:4 + W]                                                                # a column window of a wider tensor
    mwide = torch.zeros(B, 1, H + 3, W + 2, dtype=torch.bool, device="cuda")
    mwide[:, :, 1:1 + H, 2:] = masks.cuda()
    m_nc = mwide[:, :, 1:1 + H, 2:]                                                          # a bool view
    assert not g_nc.is_contiguous() and not p_nc.is_contiguous() and not m_nc.is_contiguous()
    variants = {"views": (g_nc, p_nc, m_nc, th),
                "mask_bhw_float": (gts.cuda(), preds.cuda(), masks.cuda()[:, 0].float() * 3.0, th),
                "double_inputs_tensor_thresholds": (gts.cuda().double(), preds.cuda().double(), masks.cuda().to(torch.uint8),
                                                    torch.tensor(th, dtype=torch.float64, device="cuda"))}
    for tag, args in variants.items():
        got = _to_numpy(eval_ops.eval_3d_batch(*args))
        for k in er.KEYS:
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), (tag, k)
        assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["size"], ref["size"]), tag
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        eval_ops.eval_3d_batch(gts.cuda(), preds, masks.cuda(), th)


def test_no_host_sync_and_graph_capture():
    """nothing synchronises (torch's sync debug mode raises on any), and the whole call is capturable as one chain of launches on a
    side stream (a capture fails on a synchronisation or a device-to-host copy); the replay reproduces the eager bits"""
    from unidepth_amd import eval_ops
    gts, preds, masks, th = (t.cuda() for t in er.case_inputs("small_t100"))
    ref = _gpu_case("small_t100")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = eval_ops.eval_3d_batch(gts, preds, masks, th)
        res16 = eval_ops.eval_3d_batch(gts.half(), preds.half(), masks, th)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = _to_numpy(res)
    for k in er.KEYS:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    assert torch.isfinite(res16["F1"]).all()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = eval_ops.eval_3d_batch(gts, preds, masks, th)
    graph.replay()
    torch.cuda.synchronize()
    got = _to_numpy(cap)
    for k in er.KEYS:
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["size"], ref["size"])


def test_metrics_accumulator_reduces_like_get_evaluation():
    from unidepth_amd import eval_ops
    acc = eval_ops.MetricsAccumulator(min_depth=0.01, max_depth=10.0)
    th = eval_ops.thresholds_3d(0.01, 10.0, device="cuda")
    depth_rows, rows3d, keep = {}, {k: [] for k in er.KEYS}, []
    for name in ("small_t100", "empty_middle"):                       # the second batch contains an empty image
        gts, preds, masks, _ = (t.cuda() if isinstance(t, torch.Tensor) else t for t in er.case_inputs(name))
        acc.accumulate_depth(gts[:, 2:3], preds[:, 2:3], masks)
        acc.accumulate_3d(gts, preds, masks)
        for k, v in eval_ops.eval_depth(gts[:, 2:3], preds[:, 2:3], masks, max_depth=10.0).items():
            depth_rows.setdefault(k, []).append(v)
        r = eval_ops.eval_3d_batch(gts, preds, masks, th)
        keep.append(r["count"] > 0)
        for k in er.KEYS:
            rows3d[k].append(r[k])
    want = {k: float(np.round(torch.cat(v).mean().item(), 5)) for k, v in depth_rows.items()}
    want.update({k: float(np.round(torch.cat(v)[torch.cat(keep)].mean().item(), 5)) for k, v in rows3d.items()})
    got = acc.get_evaluation()
    assert list(got) == list(eval_ops.EVAL_DEPTH_KEYS) + list(er.KEYS)
    assert int(torch.cat(keep).sum()) == 4 and torch.cat(keep).numel() == 5
    for k in want:
        if math.isnan(want[k]):
            assert math.isnan(got[k]), k                              # depth keys average plainly: the empty image's NaN propagates
        else:
            assert got[k] == want[k], (k, got[k], want[k])
    assert all(math.isnan(got[k]) for k in eval_ops.EVAL_DEPTH_KEYS) and all(math.isfinite(got[k]) for k in er.KEYS)
    assert acc.get_evaluation() == {}                                 # the store is empty afterwards
    gts, preds, masks, _ = (t.cuda() if isinstance(t, torch.Tensor) else t for t in er.case_inputs("small_t100"))
    acc.accumulate_3d(gts, preds, masks, name="v2")
    assert sorted(acc.get_evaluation()) == sorted(f"v2_{k}" for k in er.KEYS)
