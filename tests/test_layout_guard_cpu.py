"""Self-tests of tests/layout_guard.py on the CPU: the helper must FAIL on each planted defect below and pass on the clean result.
No kernel runs here; the defects are planted into torch results, never into a kernel."""
import importlib.util
import math
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(os.path.dirname(os.path.abspath(__file__)), "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)


def rel(a, b):          # the suite's rel-L2 bar (tests/test_kernels_gpu.py rel)
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guard_bands_and_bitwise_check(dtype):
    g = lg.guarded(37, 52, 52 + 256, dtype, offset_cols=8, device="cpu")
    assert g.view.shape == (37, 52) and g.view.stride() == (308, 1)
    assert g.buf.shape == (256 + 37 + 256, 308) and bool(torch.isnan(g.buf).all())
    g.view.copy_(torch.randn(37, 52).to(dtype))
    g.check_guards()                                                    # clean: every guard element still the sentinel
    ib = g.buf.view(lg._IVIEW[dtype])
    assert int(ib[0, 0]) == lg.SENTINEL[dtype] and int(ib[-1, -1]) == lg.SENTINEL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guard_catches_a_quieted_nan(dtype):
    """The sentinel is a signalling NaN: a kernel that loads and stores it back (e.g. a spilled read-modify-write) quiets it.  Equality of
    floats could not see that (NaN != NaN everywhere); the bitwise check does."""
    g = lg.guarded(20, 16, 24, dtype, device="cpu")
    g.view.zero_()
    g.buf[256 + 3, 16] = g.buf[256 + 3, 16] + 0                         # arithmetic on the sentinel: quiet NaN with the same payload
    assert bool(torch.isnan(g.buf[256 + 3, 16]))
    assert int(g.buf.view(lg._IVIEW[dtype])[256 + 3, 16]) != lg.SENTINEL[dtype]
    with pytest.raises(AssertionError, match="guard element"):
        g.check_guards()


@pytest.mark.parametrize("where", ["right", "below", "above", "wrap"])
def test_guard_catches_the_neighbours_value(where):
    """A one-vector spill past an edge tile writes the in-bounds neighbour's value, which is a perfectly good float: caught wherever it lands."""
    g = lg.guarded(40, 36, 36 + 256, torch.float32, offset_cols=4, device="cpu")
    g.view.copy_(torch.randn(40, 36))
    r, c = {"right": (256 + 7, 4 + 36), "below": (256 + 40, 4 + 5), "above": (255, 4 + 5), "wrap": (256 + 8, 3)}[where]
    g.buf[r, c] = g.buf[min(max(r, 256), 256 + 39), min(max(c, 4), 39)]
    with pytest.raises(AssertionError, match="guard element"):
        g.check_guards()


def test_dropped_k_slice_passes_rel_l2_but_not_the_elementwise_bound():
    """One 16 x 16 block of an 11008 x 1024, K = 4096 product loses one 64-wide K-slice (a skipped MFMA chain on one edge tile): that block
    is off by ~12 %, the whole output's rel-L2 stays ~6e-4 < 1e-3 (the suite's bar passes it), the element-wise bound catches it.  The same
    run calibrates C_ACC: the clean fp32 result stays well inside the bound."""
    torch.manual_seed(0)
    M, N, K = 11008, 1024, 4096
    A = torch.randn(M, K).half().float()
    W = (torch.randn(N, K) * K ** -0.5).half().float()
    out = A @ W.t()                                                     # fp32 accumulation of fp16-rounded operands
    ref = A.double() @ W.double().t()
    mag = A.double().abs() @ W.double().abs().t()
    ratio = ((out.double() - ref).abs() / (math.sqrt(K) * 2.0 ** -24 * mag)).max().item()
    assert ratio < lg.C_ACC / 4, ratio                                  # calibration: the clean fp32 sum uses a small part of the bound
    lg.assert_elementwise(out, ref, mag, K)                             # clean: passes
    lg.assert_elementwise(out.half(), ref, mag, K, fp16_out=True)       # clean fp16 store: passes
    r0, c0, k0 = M - 16, N - 16, 2048                                   # the last (edge) 16 x 16 block, K-slice [2048, 2112)
    bad = out.clone()
    bad[r0:, c0:] -= A[r0:, k0:k0 + 64] @ W[c0:, k0:k0 + 64].t()
    blk = (bad[r0:, c0:].double() - ref[r0:, c0:]).norm() / ref[r0:, c0:].norm()
    assert blk > 0.05                                                   # the block itself is badly wrong ...
    assert rel(bad, ref) < 1e-3 and rel(bad.half(), ref) < 1e-3         # ... and the suite's rel-L2 bar does not see it
    with pytest.raises(AssertionError, match=r"tile \(687, 63\)"):      # the element-wise bound does, and names the tile
        lg.assert_elementwise(bad, ref, mag, K)
    with pytest.raises(AssertionError, match="outside the bound"):
        lg.assert_elementwise(bad.half(), ref, mag, K, fp16_out=True)


def test_nan_through_a_poisoned_padding_column():
    """A strided A operand whose padding columns hold NaN: a product that reads one padding column into the reduction (an off-by-one K
    extent, a wrong lda) returns NaN, and the bound reports it; the correct product of the same view passes."""
    torch.manual_seed(1)
    M, N, K, lda = 50, 24, 64, 64 + 32
    A = lg.poisoned(torch.randn(M, K).half(), ld=lda, post_rows=3)
    W = (torch.randn(N, K) * K ** -0.5).half()
    assert A.stride() == (lda, 1) and bool(torch.isnan(torch.as_strided(A, (M, lda), (lda, 1))[:, K:]).all())
    good = A.float() @ W.float().t()
    ref = A.double() @ W.double().t()
    mag = A.double().abs() @ W.double().abs().t()
    lg.assert_elementwise(good, ref, mag, K)
    wide = torch.as_strided(A, (M, K + 1), (lda, 1))                    # reads column K: padding
    Wz = torch.cat([W, torch.zeros(N, 1, dtype=W.dtype)], 1)            # ... even against a zero weight column: NaN * 0 = NaN
    bad = wide.float() @ Wz.float().t()
    assert bool(torch.isnan(bad).all())
    with pytest.raises(AssertionError, match="outside the bound"):
        lg.assert_elementwise(bad, ref, mag, K)
    past = torch.as_strided(A, (M + 1, K), (lda, 1))                    # and a row past M holds poison too
    assert bool(torch.isnan(past[M]).all())
