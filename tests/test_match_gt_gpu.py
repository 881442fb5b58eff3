"""GPU tests of ud_match_gt (csrc/matchgt.hip, unidepth_amd/matching.py) against the numpy fp32 restatement of
tools/make_golden_match_gt.py (pinned to the reference's own arrays by tests/test_match_gt_cpu.py): every destination sits inside a
sentinel-filled guard allocation (tests/layout_guard.py), results are compared bit for bit, guards must be intact.  The shapes are the
kernel's seams, not the workload's: rows that start 0..3 elements past a 16-byte boundary (scalar head / vector body / tail), rows
shorter than a quad, windows of one row / one column, 1 x 1 windows, per-image paddings, the zero border of target paddings."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import layout_guard as lg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_match_gt", os.path.join(ROOT, "tools", "make_golden_match_gt.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rnd(rng, *shape):
    return (rng.random(shape, dtype=np.float32) * 5.0 - 1.0).astype(np.float32)


def _pads(rng, B, h, w, frac):
    return np.stack([rng.integers(0, w // frac + 1, B), rng.integers(0, w // frac + 1, B),
                     rng.integers(0, h // frac + 1, B), rng.integers(0, h // frac + 1, B)], axis=1)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _run(planes, B, h1, w1, H2, W2, p1=None, p2=None, K=None, off=0):
    """One ud_match_gt on guarded destinations (plane i starts (off + i) % 4 elements past a 16-byte boundary), compared bitwise with
    restate() / restate_intrinsics().  planes: (src [nb,C,h1,w1], mul [B,1,h1,w1] or None) numpy pairs."""
    from unidepth_amd import matching
    dev = "cuda"
    descs, dsts, keep = [], [], []
    for i, (src, mul) in enumerate(planes):
        nb, Cn = src.shape[:2]
        n = B * Cn * H2 * W2
        g = lg.guarded(1, n, (n + 131) // 4 * 4, torch.float32, pre_rows=1, post_rows=1, offset_cols=32 + (off + i) % 4)
        s = torch.from_numpy(src).to(dev)
        m = None if mul is None else torch.from_numpy(mul).to(dev)
        keep += [s, m]
        d = dict(src=s, dst=g.ptr(), C=Cn, src_batch_stride=0 if (nb == 1 and B > 1) else Cn * h1 * w1)
        if m is not None:
            d["mul"] = m
        descs.append(d)
        dsts.append(g)
    d1, d2 = matching.upload_paddings(None if p1 is None else [tuple(int(v) for v in r) for r in p1],
                                      None if p2 is None else [tuple(int(v) for v in r) for r in p2], dev)
    Kin = Kout = None
    if K is not None:
        Kin = torch.from_numpy(K).to(dev)
        Kout = lg.guarded(1, B * 9, B * 9 + 64, torch.float32, pre_rows=1, post_rows=1, offset_cols=17)
    matching.launch(descs, B, h1, w1, H2, W2, d1, d2, Kin, None if Kout is None else Kout.view)
    torch.cuda.synchronize()
    for i, ((src, mul), g) in enumerate(zip(planes, dsts)):
        got = g.view.cpu().numpy().reshape(B, src.shape[1], H2, W2)
        ref = mg.restate(src, H2, W2, p1, p2, mul=mul, B=B, dtype=np.float32)
        if not _bits_equal(got, ref):
            bad = np.argwhere(got.view(np.int32) != ref.view(np.int32))
            raise AssertionError(f"plane {i}: {len(bad)} element(s) differ from the fp32 restatement; first at {tuple(bad[0])}: "
                                 f"{got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}")
    if K is not None:
        refK = mg.restate_intrinsics(K, (h1, w1), (H2, W2), p1, p2)
        assert _bits_equal(Kout.view.cpu().numpy().reshape(B, 3, 3), refK)
        dsts.append(Kout)
    lg.check_guards(*dsts)


# (h1, w1, H2, W2): up, down, mixed (up in y, down in x), identity; destination rows of 1, 5, 63, 65 and 257 pixels and one multiple of 4;
# source windows of one row and of one column
SHAPES = [(28, 42, 37, 53), (42, 56, 20, 31), (14, 70, 33, 17), (28, 42, 28, 42), (9, 11, 1, 1), (9, 11, 5, 63), (30, 90, 7, 65),
          (9, 11, 3, 257), (12, 20, 8, 64), (1, 17, 6, 9), (13, 1, 6, 9)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
@pytest.mark.parametrize("B", [1, 3])
def test_planes_bitwise_and_guards(shape, B):
    """four variants per shape: (0) no paddings, C = 1; (1) random per-image source paddings, a `mul` plane and a broadcast source, C = 3,
    intrinsics; (2) source paddings on one side / all zero / random plus target paddings; (3) the largest legal source padding (a 1 x 1
    window) with target paddings, four planes, intrinsics"""
    h1, w1, H2, W2 = shape
    rng = np.random.default_rng(1000 * B + h1 * 7 + W2)
    # 0
    _run([(_rnd(rng, B, 1, h1, w1), None)], B, h1, w1, H2, W2, off=0)
    # 1
    p1 = _pads(rng, B, h1, w1, 3)
    planes = [(_rnd(rng, B, 3, h1, w1), _rnd(rng, B, 1, h1, w1)), (_rnd(rng, 1, 3, h1, w1), _rnd(rng, B, 1, h1, w1) if B > 1 else None)]
    _run(planes, B, h1, w1, H2, W2, p1, None, K=_rnd(rng, B, 3, 3) * 20.0, off=1)
    # 2
    p1 = _pads(rng, B, h1, w1, 3)
    p1[0] = [min(3, w1 - 1), 0, 0, 0]
    if B > 1:
        p1[1] = [0, 0, 0, 0]
    _run([(_rnd(rng, B, 1, h1, w1), None)], B, h1, w1, H2, W2, p1, _pads(rng, B, H2, W2, 4), off=2)
    # 3
    p1 = _pads(rng, B, h1, w1, 3)
    p1[0] = [w1 - 1, 0, 0, h1 - 1]
    planes = [(_rnd(rng, B, 1, h1, w1), None), (_rnd(rng, B, 3, h1, w1), _rnd(rng, B, 1, h1, w1)), (_rnd(rng, 1, 2, h1, w1), None),
              (_rnd(rng, B, 1, h1, w1), None)]
    _run(planes, B, h1, w1, H2, W2, p1, _pads(rng, B, H2, W2, 4), K=_rnd(rng, B, 3, 3) * 20.0, off=3)


def test_identity_windows_are_bit_copies():
    """paddings that make the two windows equal (differently per image): a copy of the window, -0, inf and NaN included, and of the
    rounded product with `mul`; the zero border of the target paddings is exact"""
    rng = np.random.default_rng(7)
    src = _rnd(rng, 2, 2, 20, 30)
    src[0, 0, 3, 4], src[0, 1, 5, 6], src[1, 0, 7, 8] = -0.0, np.inf, np.nan
    with np.errstate(all="ignore"):
        prod = src.copy()
        prod[1, 0, 7, 8] = 2.5                         # the payload of a NaN product is not part of the definition
        _run([(src, None), (prod, _rnd(rng, 2, 1, 20, 30))], 2, 20, 30, 16, 26, np.array([[2, 2, 1, 3], [0, 4, 4, 0]]), None, K=_rnd(rng, 2, 3, 3))
        _run([(src, None)], 2, 20, 30, 20, 30, np.array([[2, 2, 1, 3], [0, 4, 4, 0]]), np.array([[2, 2, 1, 3], [1, 3, 2, 2]]))


def test_intrinsics_only():
    rng = np.random.default_rng(9)
    _run([], 3, 20, 30, 16, 26, _pads(rng, 3, 20, 30, 3), _pads(rng, 3, 16, 26, 4), K=_rnd(rng, 3, 3, 3) * 30.0)


def test_98x126_to_480x640():
    rng = np.random.default_rng(11)
    B = 2
    planes = [(_rnd(rng, B, 3, 98, 126), _rnd(rng, B, 1, 98, 126)), (_rnd(rng, B, 1, 98, 126), None)]
    _run(planes, B, 98, 126, 480, 640, _pads(rng, B, 98, 126, 3), None, K=_rnd(rng, B, 3, 3) * 50.0)


def test_paddings_outside_the_maps_are_clamped():
    """the C-ABI cannot validate device arrays: whatever they hold, every source index stays inside the allocation (no fault, finite
    results from finite sources) and nothing outside the destinations is written"""
    from unidepth_amd import matching
    rng = np.random.default_rng(13)
    B, h1, w1, H2, W2 = 2, 20, 30, 7, 9
    src = torch.from_numpy(_rnd(rng, B, 2, h1, w1)).cuda()
    for p1, p2 in (([[-5, 1000, 7, -3], [1 << 30, 1 << 30, -(1 << 30), 5]], [[99, 99, 99, 99], [-1, -1, -1, -1]]),
                   ([[29, 29, 19, 19], [30, 0, 20, 0]], None)):
        n = B * 2 * H2 * W2
        g = lg.guarded(1, n, n + 128, torch.float32, pre_rows=1, post_rows=1, offset_cols=33)
        d1 = torch.tensor(p1, dtype=torch.int32, device="cuda")
        d2 = None if p2 is None else torch.tensor(p2, dtype=torch.int32, device="cuda")
        matching.launch([dict(src=src, dst=g.ptr(), C=2, src_batch_stride=2 * h1 * w1)], B, h1, w1, H2, W2, d1, d2)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g.view).all())
        g.check_guards()


# ---- the Python surface --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mg.GOLDEN_CASES)
def test_match_gt_and_match_intrinsics_on_golden_cases(name):
    """the public functions on the golden cases: bit-equal to the fp32 restatement, inside the CPU test's bound of the reference's own
    output; paddings as tensors and as lists; fp16 in, fp16 out"""
    from unidepth_amd import match_gt, match_intrinsics
    src, p1, p2, K, (H2, W2) = mg.case_inputs(name)
    B, _, h1, w1 = src.shape
    t1, t2 = torch.from_numpy(src).cuda(), torch.empty(B, 1, H2, W2, device="cuda")
    pt1 = torch.from_numpy(p1).cuda()
    pl2 = None if p2 is None else [tuple(int(v) for v in r) for r in p2]
    out = match_gt(t1, t2, pt1, pl2)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, src.shape[1], H2, W2)
    r32 = mg.restate(src, H2, W2, p1, p2, dtype=np.float32)
    assert _bits_equal(out.cpu().numpy(), r32)
    g = np.load(mg.GOLDEN)
    r64 = torch.from_numpy(mg.restate(src, H2, W2, p1, p2, dtype=np.float64))
    mag = torch.from_numpy(mg.restate(np.abs(src), H2, W2, p1, p2, dtype=np.float64))
    taps = torch.from_numpy(mg.restate(src, H2, W2, p1, p2, dtype=np.float64, what="tapsum"))
    coord = max(max(h1 - int(p1[b, 2]) - int(p1[b, 3]), w1 - int(p1[b, 0]) - int(p1[b, 1])) for b in range(B))
    bound = lg.term_rounding(mag, 4) + lg.term_coord(coord, taps)
    lg.assert_bound(out.cpu(), r64, bound, name=name)
    lg.assert_bound(torch.from_numpy(g[name + ".out"]), r64, bound, name=name + " (reference)")
    Kn = match_intrinsics(torch.from_numpy(K).cuda(), t1, t2, [tuple(int(v) for v in r) for r in p1], None if p2 is None else torch.from_numpy(p2))
    assert _bits_equal(Kn.cpu().numpy(), g[name + ".K"])
    half = match_gt(t1.half(), t2, pt1, pl2)
    assert half.dtype == torch.float16
    assert torch.equal(half.cpu(), torch.from_numpy(mg.restate(t1.half().float().cpu().numpy(), H2, W2, p1, p2)).half())


def test_eval_depth_of_matched_prediction_equals_eval_depth_of_prediction():
    """with zero paddings match_gt is eval_depth's own resample: the 18 metrics agree bit for bit"""
    from unidepth_amd import match_gt
    from unidepth_amd.eval_ops import eval_depth
    g = torch.Generator().manual_seed(3)
    B, h, w, H, W = 2, 28, 42, 37, 53
    gt = (1.0 + 6.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
    pred = (1.0 + 6.0 * torch.rand(B, 1, h, w, generator=g)).cuda()
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.8).cuda()
    a = eval_depth(gt, match_gt(pred, gt, None, None), mask)
    b = eval_depth(gt, pred, mask)
    torch.cuda.synchronize()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_calls_are_reproducible():
    from unidepth_amd import match_gt
    src, p1, p2, _, (H2, W2) = mg.case_inputs("up_28x42_63x257_pads2")
    t1, t2 = torch.from_numpy(src).cuda(), torch.empty(src.shape[0], 1, H2, W2, device="cuda")
    a, b = match_gt(t1, t2, p1.tolist(), p2.tolist()), match_gt(t1, t2, p1.tolist(), p2.tolist())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
