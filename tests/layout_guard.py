"""Layout / guard helpers of the kernel tests (not a conftest: the test modules import it, like they import tools).

The kernel suite's plain cases run on dense operands, outputs exactly as wide as the result and zero-filled buffers, judged by one
rel-L2 number.  The product does not work that way (strided token rows, interleaved column slices, padded row blocks), so these
helpers put every operand and output of a call inside a larger allocation:

  guarded(...)   an OUTPUT view inside an allocation whose every other element holds a signalling-NaN bit pattern (fp32 0x7FBADBAD,
                 fp16 0x7D5A).  Arithmetic would quiet it, so any write outside the view -- even of a NaN or of the neighbour's own
                 value -- changes the bits; check_guards() compares every guard element bitwise.  The bands are at least one tile
                 (256 rows) above and below, and `ld - cols` columns to the right of every row.
  poisoned(...)  the same for INPUTS: the data sits in a view, the padding columns (ld > width), the rows past the logical extent and
                 the channels past Cin hold a quiet NaN, so a kernel that lets padding into a result returns NaN.  Padding that the
                 C-ABI requires to be zero (W's K padding, V^T columns in [Nk, kv_ld), the `zeros` buffer) is built by the caller.
  assert_elementwise(out, ref64, mag64, K, ...)
                 every element, not one norm:  |out - ref| <= r_out |ref| + c sqrt(K) 2^-24 mag (+ r_mag mag + atol), where ref64 is
                 the fp64 result on the same fp16-rounded operands and mag64 the same expression on absolute values.

C_ACC (the c above) was calibrated in tests/test_layout_guard_cpu.py: an fp32 GEMM of fp16-rounded random operands (11008 x 1024,
K = 4096) against its fp64 value reaches at most ~0.015 sqrt(K) 2^-24 mag per element (blocked fp32 sums, the test asserts < c / 4).  A
GPU kernel's fp32 chains are longer and sequential per MFMA accumulator (a random walk whose tail over ~10^7 elements is ~5 sigma), so
c = 8 keeps a wide margin for every schedule, while a dropped 64-wide K-slice (error ~ |A_s||W_s| ~ 1 for the unit-variance product of
that test) still exceeds the bound (~0.01 there) by two orders of magnitude.
"""
from __future__ import annotations

import math

import torch

SENTINEL = {torch.float32: 0x7FBADBAD, torch.float16: 0x7D5A}       # signalling NaNs: quiet bit clear, non-zero payload
QNAN = {torch.float32: 0x7FC00000, torch.float16: 0x7E00}
_IVIEW = {torch.float32: torch.int32, torch.float16: torch.int16}
C_ACC = 8.0
GELU_SLOPE = 1.13          # max |d GELU / dx|: an accumulation error behind the exact-erf GELU grows by at most this factor
GUARD_ROWS = 256


def vt_cols(n):
    """Column of key t in the V^T layout of ud_attention_f16 (include/unidepth_hip.h): the 4-key blocks of every aligned 16-key group in
    the order [0, 2, 1, 3].  A host tensor; the permutation is its own inverse."""
    t = torch.arange(n)
    return (t & ~15) | ((t & 4) << 1) | ((t & 8) >> 1) | (t & 3)


def _bits(dtype, pattern):
    return pattern          # every pattern above is positive as a signed integer of its width


def _filled(n, dtype, pattern, device):
    buf = torch.empty(n, dtype=dtype, device=device)
    buf.view(_IVIEW[dtype]).fill_(_bits(dtype, pattern))
    return buf


class Guarded:
    """An output view [rows, cols] with row stride `ld` at (pre_rows, offset_cols) inside a sentinel-filled [pre + rows + post, ld] allocation."""

    def __init__(self, rows, cols, ld, dtype, pre_rows=GUARD_ROWS, post_rows=GUARD_ROWS, offset_cols=0, device="cuda", init=None, rows_inside=None):
        assert ld >= offset_cols + cols, (ld, offset_cols, cols)
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.pre, self.post, self.off = pre_rows, post_rows, offset_cols
        self.buf = _filled((pre_rows + rows + post_rows) * ld, dtype, SENTINEL[dtype], device).view(pre_rows + rows + post_rows, ld)
        self.view = self.buf[pre_rows:pre_rows + rows, offset_cols:offset_cols + cols]
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
        self.rows_inside = rows_inside
        if rows_inside is None:                     # rows_inside: the view's rows the op may write (others are guard rows inside the view)
            self.inside[pre_rows:pre_rows + rows, offset_cols:offset_cols + cols] = True
            if init is not None:
                self.view.copy_(init)
        else:
            self.inside[pre_rows + rows_inside, offset_cols:offset_cols + cols] = True
            if init is not None:
                self.view[rows_inside] = init[rows_inside].to(dtype)

    def ptr(self):
        return self.view.data_ptr()

    def written(self):
        """The part of the view the op may write (rows_inside), for bit-identity comparisons between layouts."""
        return self.view if self.rows_inside is None else self.view[self.rows_inside]

    def check_guards(self, name="output"):
        """Every element outside the view still holds the sentinel, compared bitwise."""
        bits = self.buf.view(_IVIEW[self.dtype])
        bad = (bits != _bits(self.dtype, SENTINEL[self.dtype])) & ~self.inside
        n = int(bad.sum())
        if n:
            r, c = [int(v) for v in bad.nonzero()[0]]
            raise AssertionError(f"{name}: {n} guard element(s) rewritten; first at buffer row {r - self.pre} (view-relative), column "
                                 f"{c - self.off} (view-relative; view is {self.rows} x {self.cols}, ld {self.ld}); bits "
                                 f"0x{int(bits[r, c]) & ((1 << (8 * self.buf.element_size())) - 1):x}")


def guarded(rows, cols, ld, dtype, pre_rows=GUARD_ROWS, post_rows=GUARD_ROWS, offset_cols=0, device="cuda", init=None, rows_inside=None):
    return Guarded(rows, cols, ld, dtype, pre_rows, post_rows, offset_cols, device, init, rows_inside)


def check_guards(*gs):
    for i, g in enumerate(gs):
        g.check_guards(f"output {i}")


def poisoned(data, ld=None, pre_rows=0, post_rows=0, offset_cols=0, fill=None):
    """`data` [rows, cols] copied into a view with row stride `ld` at (pre_rows, offset_cols) of an allocation whose other elements hold
    a quiet NaN (or `fill`): padding columns and the `post_rows` rows past the logical extent are poison.  Returns the view."""
    rows, cols = data.shape
    ld = cols if ld is None else ld
    assert ld >= offset_cols + cols
    n = (pre_rows + rows + post_rows) * ld
    if fill is None:
        buf = _filled(n, data.dtype, QNAN[data.dtype], data.device)
    else:
        buf = torch.full((n,), fill, dtype=data.dtype, device=data.device)
    buf = buf.view(pre_rows + rows + post_rows, ld)
    v = buf[pre_rows:pre_rows + rows, offset_cols:offset_cols + cols]
    v.copy_(data)
    return v


# ---- bounds as sums of named terms (the pointwise / resampling kernels, tests/test_pointwise_layouts_gpu.py) ----------------------------
# assert_elementwise above is one formula for fp32 reduction chains; the kernels outside the GEMM family have other error sources
# (source coordinates computed in fp32, transcendentals, an fp16 store behind a LayerNorm), so their bound is built per case as a SUM
# of the terms below, each a tensor shaped like the result, and checked by assert_bound.  Nothing here depends on a kernel's output.
def term_rounding(mag64, taps):
    """fp32 products and sums over `taps` terms: C_ACC sqrt(taps) 2^-24 mag, mag = the same expression on absolute values."""
    return C_ACC * math.sqrt(max(taps, 1)) * 2.0 ** -24 * mag64.double()


def term_coord(max_coord, tap_abs_sum64):
    """Source coordinates computed in fp32: a coordinate near `max_coord` carries ~2^-24 max_coord of rounding per operation (scale,
    product, floor subtraction), the interpolation weight inherits it, and the result moves by delta_w |v1 - v0| <= delta_w sum |taps|.
    `mag` can be near zero where the taps cancel, so the term is max_coord 2^-22 sum |tap values|, not a multiple of mag."""
    return float(max_coord) * 2.0 ** -22 * tap_abs_sum64.double()


def term_store_f16(ref64):
    """Round-to-nearest fp16 store: 2^-11 |ref|, plus half the subnormal spacing."""
    return 2.0 ** -11 * ref64.double().abs() + 2.0 ** -25


def term_store_f32(ref64):
    """ONE correctly rounded fp32 operation (half a unit in the last place, 2^-24 |ref|) under the factor-4 headroom rule: 2^-22 |ref|."""
    return 2.0 ** -22 * ref64.double().abs()


def bound_ratio(out, ref64, bound64):
    """max over the elements of |out - ref| / bound (inf where out is NaN or the bound is zero and the error is not)."""
    o = out.double().reshape(ref64.shape)
    err = (o - ref64.double()).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    b = bound64.double().expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return ratio, err


def assert_bound(out, ref64, bound64, name="result", margin=1.0):
    """|out - ref| * margin <= bound for EVERY element; returns the worst error / bound.  margin = 4 is the headroom rule of C_ACC (the
    clean fp32 evaluation uses at most a quarter of the bound)."""
    if ref64.numel() == 0:
        return 0.0
    ratio, err = bound_ratio(out, ref64, bound64)
    worst = int(ratio.reshape(-1).argmax())
    w = float(ratio.reshape(-1)[worst])
    if not w * margin <= 1.0:
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(worst), ratio.shape))
        n = int((ratio * margin > 1.0).sum())
        raise AssertionError(f"{name}: {n} element(s) outside the bound{'' if margin == 1.0 else f' / {margin:g}'}; worst at {idx}: out "
                             f"{out.double().reshape(ref64.shape).reshape(-1)[worst].item():.8g}, ref {ref64.double().reshape(-1)[worst].item():.8g}, "
                             f"error {err.reshape(-1)[worst].item():.3g} > bound {bound64.double().expand_as(err).reshape(-1)[worst].item():.3g}")
    return w


def assert_elementwise(out, ref64, mag64, K, fp16_out=False, c=C_ACC, gelu=False, r_mag=0.0, atol=0.0, tile=(16, 16), name="result"):
    """|out - ref| <= r_out |ref| + g (c sqrt(K) 2^-24 + r_mag) mag + atol for EVERY element (g = 1.13 behind GELU, r_out = 2^-11 for fp16
    stores, plus the fp16 subnormal spacing).  On failure: the worst element's (row, column), the tile it falls in and its numbers.
    Returns the worst error / bound."""
    o = out.double().reshape(ref64.shape[0], -1) if out.dim() != ref64.dim() else out.double()
    ref = ref64.double().reshape(o.shape)
    mag = mag64.double().reshape(o.shape)
    g = GELU_SLOPE if gelu else 1.0
    r_out = 2.0 ** -11 if fp16_out else 0.0
    bound = r_out * ref.abs() + g * (c * math.sqrt(max(K, 1)) * 2.0 ** -24 + r_mag) * mag + atol + (2.0 ** -25 if fp16_out else 0.0)
    err = (o - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    excess = err / bound
    worst = excess.reshape(-1).argmax().item() if excess.numel() else 0
    if excess.numel() and not bool((err <= bound).all()):
        o2 = excess.reshape(excess.shape[0], -1) if excess.dim() > 1 else excess.reshape(1, -1)
        r, col = divmod(worst, o2.shape[1])
        n = int((err > bound).sum())
        raise AssertionError(f"{name}: {n} element(s) outside the bound; worst at (row {r}, column {col}) = tile ({r // tile[0]}, {col // tile[1]}) "
                             f"of {tile[0]}x{tile[1]}: out {o.reshape(-1)[worst].item():.6g}, ref {ref.reshape(-1)[worst].item():.6g}, "
                             f"error {err.reshape(-1)[worst].item():.3g} > bound {bound.reshape(-1)[worst].item():.3g}")
    return float(excess.reshape(-1)[worst]) if excess.numel() else 0.0
