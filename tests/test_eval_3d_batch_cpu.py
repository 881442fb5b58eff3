"""eval_3d_batch without a GPU (unidepth_amd/eval_ops.py, include/unidepth_hip.h UdEval3d): the size rule and the thresholds against the
reference's torch expressions, the numpy restatement of tests/eval3d_restate.py against the reference's own outputs
(tests/golden/eval_3d_batch.npz), the C-ABI's descriptor, argument checks and workspace query, and eval_3d_batch's argument errors."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval3d_restate as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_size(H, W, S):
    """utils/evaluation_depth.py:164-165 on a CPU tensor: the ratio is an fp32 tensor (or the Python float 1.0)."""
    ratio = min(1.0, (240 * 320 / torch.tensor(S)) ** 0.5)
    return int(H * ratio), int(W * ratio)


def test_eval_3d_size_is_the_reference_expression():
    from unidepth_amd import eval_ops
    assert eval_ops.eval_3d_size(518, 518, 804972) == (160, 160)             # an fp64 product gives 159
    assert eval_ops.eval_3d_size(518, 518, 201243) == (320, 320)             # an fp64 product gives 319
    assert eval_ops.eval_3d_size(240, 320, 76800) == (240, 320)
    assert eval_ops.eval_3d_size(240, 320, 76801) == _reference_size(240, 320, 76801) == (239, 319)
    assert eval_ops.eval_3d_size(100, 100, 80000) == (97, 97)
    assert eval_ops.eval_3d_size(37, 53, 0) == (37, 53)
    g = torch.Generator().manual_seed(1)
    sweep = [(518, 518, 804972), (518, 518, 201243), (240, 320, 76800), (240, 320, 76801), (1, 1, 1), (1, 90000, 90000), (3, 5, 15)]
    for H, W in ((240, 320), (480, 640), (518, 518), (375, 1242), (260, 340), (1080, 1920), (37, 53), (644, 966)):
        for B in (1, 2, 3, 8):
            hi = B * H * W
            sweep += [(H, W, hi), (H, W, max(1, hi - 1)), (H, W, 76799), (H, W, 76800), (H, W, 76801)]
            sweep += [(H, W, int(s)) for s in torch.randint(1, hi + 1, (40,), generator=g)]
    for H, W, S in sweep:
        if S > H * W * 8:
            continue
        assert eval_ops.eval_3d_size(H, W, S) == _reference_size(H, W, S), (H, W, S)


def test_nearest_exact_index_is_interpolates():
    for n_in, n_out in ((100, 97), (518, 160), (518, 320), (260, 205), (37, 37), (53, 1), (7, 3), (640, 639)):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        want = F.interpolate(src, size=(n_out, 1), mode="nearest-exact").view(-1).long().numpy()
        np.testing.assert_array_equal(er.nearest_exact_index(n_in, n_out), want)


def test_thresholds_3d_is_the_reference_expression():
    from unidepth_amd import eval_ops
    for lo, hi in ((0.01, 10.0), (0.01, 1000.0), (0.5, 80.0)):
        want = torch.linspace(math.log(lo), math.log(hi / 20), steps=100).exp()
        got = eval_ops.thresholds_3d(lo, hi)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    assert eval_ops.EVAL_3D_KEYS == er.KEYS


def test_golden_has_every_case():
    g = np.load(er.GOLDEN)
    assert sorted(g.files) == sorted(f"{c}.{k}" for c in er.CASES for k in er.KEYS)
    rows = {"small_t100": 2, "empty_middle": 2, "edge_b8_100": 8, "full_518_b3": 3, "quarter_518_b3": 3, "ties_lattice": 2}
    for c in er.CASES:
        for k in er.KEYS:
            assert g[f"{c}.{k}"].dtype == np.float32 and g[f"{c}.{k}"].shape == (rows[c],)
    assert os.path.getsize(er.GOLDEN) < 16 * 1024


@pytest.mark.parametrize("name", er.CASES)
def test_restatement_matches_reference_golden(name):
    """the restatement (NaN rows of empty images dropped, as the reference skips them) against the reference's own eval_3d, within the
    tolerance tests/test_eval_ops_gpu.py uses for eval_3d against the same reference"""
    r = er.restated_case(name)
    gts, _, masks, _ = er.case_inputs(name)
    assert r["size"] == _reference_size(gts.shape[-2], gts.shape[-1], int(masks.sum()))
    keep = r["count"] > 0
    ref = er.golden(name)
    for k in er.KEYS:
        assert not np.isnan(r[k][keep]).any() and np.isnan(r[k][~keep]).all()
        np.testing.assert_allclose(r[k][keep], ref[k], rtol=er.RTOL, atol=0, err_msg=f"{name}.{k}")


def test_case_properties():
    """every case exercises what it is there for"""
    assert er.restated_case("small_t100")["size"] == (48, 64)
    r = er.restated_case("empty_middle")
    assert r["count"][1] == 0 and r["count"][2] == 1 and r["count"][0] > 1 and r["size"] == (37, 53)
    r = er.restated_case("edge_b8_100")
    assert r["size"] == (97, 97) and r["count"].tolist() == [97 * 97] * 8
    r = er.restated_case("full_518_b3")
    assert r["size"] == (160, 160) and r["count"].tolist() == [160 * 160] * 3
    r = er.restated_case("quarter_518_b3")
    assert r["size"] == (320, 320) and r["count"][0] > 1.5 * r["count"][1] > 3 * r["count"][2] > 0
    r = er.restated_case("ties_lattice")
    # squared distances 0, 1 and 2..3 all occur: ties with the thresholds 1 and 2
    assert (np.diff(r["c1"], axis=1) > 0).all() and (np.diff(r["c2"], axis=1) > 0).all()
    g, p, m, th = er.case_inputs("ties_lattice")
    assert th == [1.0, 2.0, 4.0] and float((g - g.round()).abs().max()) == 0.0


def test_many_tiles_inputs_reach_the_second_chunk_of_the_scan():
    """the input of test_eval_3d_batch_gpu's 263-tile case (its own assertions: the tiles that hold valid pixels, no resampling)"""
    from unidepth_amd import eval_ops
    gts, preds, masks, th = er.many_tiles_inputs()
    n = masks.flatten(1).sum(1).tolist()
    assert gts.shape == (2, 3, 518, 518) and all(2900 < k < 3100 for k in n) and eval_ops.eval_3d_size(518, 518, sum(n)) == (518, 518)


def test_f1_from_counts():
    assert er.f1_from_counts([5], [5], 10) == 0.0                                            # T = 1: an empty trapezoid
    assert er.f1_from_counts([0, 0], [0, 0], 7) == 0.0                                       # 0 / 0 -> 0
    assert er.f1_from_counts([10, 10], [10, 10], 10) == np.float32(0.5)                      # f = 1, 1: area 1, / T
    assert er.f1_from_counts([0, 10, 10], [0, 10, 10], 10) == np.float32(1.5 / 3)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------

def test_eval_3d_descriptor_fields_and_threshold_limit():
    from unidepth_amd import _lib
    assert [n for n, _ in _lib.UdEval3d._fields_] == ["gt", "pred", "mask", "thresholds", "out", "counts", "size", "work", "work_bytes",
                                                      "B", "H", "W", "T"]
    assert _lib.UD_EVAL3D_MAX_T >= 128


def test_eval_3d_rejects_bad_descriptors_without_a_launch():
    """every refusal comes back before any HIP call: this runs on a machine without a GPU, the pointers are never followed"""
    from unidepth_amd import _lib
    lib = _lib.lib
    P = 0x1000                                      # stands for a device pointer
    B, H, W, T = 2, 5, 7, 100
    nbytes = lib.ud_eval_3d_work_bytes(B, H, W, T)
    assert nbytes > 0

    def rc(**kw):
        base = dict(gt=P, pred=P, mask=P, thresholds=P, out=P, counts=P, size=P, work=P, work_bytes=nbytes, B=B, H=H, W=W, T=T)
        base.update(kw)
        d = _lib.UdEval3d()
        for k, v in base.items():
            setattr(d, k, v)
        r = lib.ud_eval_3d(C.byref(d), None)
        return r, lib.ud_last_error().decode()

    r, msg = lib.ud_eval_3d(None, None), lib.ud_last_error().decode()
    assert r < 0 and "null descriptor" in msg
    for kw, word in ([(dict(**{k: None}), "null pointer") for k in ("gt", "pred", "mask", "thresholds", "out", "counts", "size", "work")] +
                     [(dict(work=P + 4), "16-byte aligned"), (dict(work_bytes=nbytes - 1), "workspace smaller"), (dict(work_bytes=0), "workspace smaller"),
                      (dict(B=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-1), "bad sizes"), (dict(T=0), "bad sizes"),
                      (dict(B=_lib.UD_EVAL3D_MAX_B + 1), "bad sizes"), (dict(T=_lib.UD_EVAL3D_MAX_T + 1), "bad sizes"),
                      (dict(H=65536, W=32768), "bad sizes"), (dict(B=64, H=32768, W=32768), "bad sizes")]):
        r, msg = rc(**kw)
        assert r < 0 and word in msg, (kw, r, msg)


def test_work_bytes_covers_the_point_rows():
    from unidepth_amd import _lib
    wb = _lib.lib.ud_eval_3d_work_bytes
    prev = 0
    for B, H, W, T in ((1, 1, 1, 1), (1, 32, 32, 100), (3, 37, 53, 100), (8, 518, 518, 100), (8, 480, 640, 100)):
        n = wb(B, H, W, T)
        assert n % 16 == 0 and n >= B * H * W * (2 * 12 + 2 * 4) + B * 2 * T * 4 and n > prev     # gt + pred rows, two distance slots
        assert wb(B, H, W, T + 1) >= n
        prev = n
    for bad in ((0, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 4, 4, _lib.UD_EVAL3D_MAX_T + 1), (1, 65536, 32768, 1)):
        assert wb(*bad) == -1


# ---- Python argument errors (raised before the device check, so they show on a machine without a GPU) ----------------------------------

def test_eval_3d_batch_argument_errors():
    from unidepth_amd import eval_ops
    gt = torch.rand(2, 3, 8, 8)
    m = torch.ones(2, 1, 8, 8, dtype=torch.bool)
    th = [0.1, 0.2]
    for args in ((gt[:, :2], gt[:, :2], m, th),                       # not 3 channels
                 (gt[0], gt[0], m, th),                               # not 4-D
                 (gt, gt[:1], m, th),                                 # batch sizes differ
                 (gt, gt[..., :7], m, th),                            # preds shape
                 (gt, gt, m[:1], th),                                 # masks batch
                 (gt, gt, m[..., :7], th),                            # masks shape
                 (gt, gt, torch.ones(2, 2, 8, 8, dtype=torch.bool), th),
                 (gt[:0], gt[:0], m[:0], th),                         # empty batch
                 (gt.long(), gt, m, th),                              # integer maps
                 (gt, gt, m, []),                                     # no threshold
                 (gt, gt, m, torch.rand(2, 2)),                       # thresholds not 1-D
                 (gt, gt, m, [0.1] * 1025),                           # above UD_EVAL3D_MAX_T
                 (gt, gt, m, 0.5),                                    # not a sequence
                 ("gt", gt, m, th)):
        with pytest.raises(ValueError):
            eval_ops.eval_3d_batch(*args)
    with pytest.raises(RuntimeError, match="GPU tensors expected"):    # well-formed CPU tensors: the device check comes last
        eval_ops.eval_3d_batch(gt, gt, m, th)
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        eval_ops.eval_3d_batch(gt, gt, m[:, 0], torch.tensor(th))
    acc = eval_ops.MetricsAccumulator()
    assert (acc.min_depth, acc.max_depth) == (0.01, 1000.0) and acc.get_evaluation() == {}
