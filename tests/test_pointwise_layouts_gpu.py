"""The launch-program kernels outside the GEMM / LayerNorm / attention family (pointwise.hip, convnext.hip, v1dec.hip) under the regime of
tests/test_kernel_layouts_gpu.py: inputs at a row stride wider than their width with NaN in the padding and in the rows past the logical
extent, outputs at an offset inside a sentinel-filled allocation, a BITWISE check of every guard element, and a bound on EVERY element
against an fp64 torch statement of the op on the same inputs.  Where the C-ABI has a dense product layout too, it runs as well and both
results must agree bit for bit.

POINTWISE_CASES is the one table of cases.  Each op is an `Op`: make (inputs, on the host), evaluate (the definition in torch at a given
dtype: fp64 is the reference, fp32 the headroom probe of tests/test_pointwise_bounds_cpu.py, keyword arguments plant the defects that
module checks the bounds against), bounds (a sum of the named terms of tests/layout_guard.py) and run (the GPU launch at one layout).
Nothing in a bound comes from a kernel's output.  The module imports without a GPU; tests/test_layout_coverage_cpu.py reads
declared_classes() and point_class() from it.

Transcendental terms (expf, sinf / cosf, the softmax exponentials): the constant T_* next to each op is 4 x the error of torch's own fp32
CPU evaluation of the same formula against fp64 on that op's cases, in the unit named there (device libm is a few ulp against glibc's ~1)."""
import contextlib
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(_here, "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)

pytestmark = pytest.mark.gpu

F32, F16, F64 = torch.float32, torch.float16, torch.float64
(K_RESIZE_AA, K_SH_EMBED, K_SOFTMAX, K_ATTN_FEWQ, K_HEAD_MIX, K_ADD, K_COPY_ROWS, K_CAMERA, K_POINTS, K_MEAN3, K_PREPROCESS, K_VIT_TAP, K_RESIZE_AC_SPLIT,
 K_OUT_CONV3) = (1, 2, 3, 4, 5, 8, 9, 11, 12, 13, 14, 15, 17, 18)          # include/unidepth_hip.h UD_V1_*
U24 = 2.0 ** -24


class Op:
    """bounds() covers the ARITHMETIC (what the fp32 headroom probe is held to a quarter of); stores: {output: "f16" | "pair"} names the outputs
    whose number format adds a term of its own -- an fp16 store, or the [hi | lo] fp16 pair standing for an fp32 value."""

    def __init__(self, make, evaluate, bounds, run, dense=False, stores=None):
        self.make, self.evaluate, self.bounds, self.run, self.dense = make, evaluate, bounds, run, dense
        self.stores = stores or (lambda c: {})


def term_store(kind, ref64):
    if kind == "f16":
        return lg.term_store_f16(ref64)
    # hi = fp16(v); lo = fp16(v - hi), v - hi exact in fp32: |v - hi - lo| <= 2^-11 |v - hi| + 2^-25 <= 2^-22 |v| + 2^-24
    return 2.0 ** -22 * ref64.double().abs() + 2.0 ** -24


OPS = {}
POINTWISE_CASES = []


def _case(op, id, cls, **kw):
    POINTWISE_CASES.append(dict(op=op, id=f"{op}-{id}", cls=(op,) + tuple(cls), **kw))


def declared_classes():
    """The coverage classes of the table (tests/test_layout_coverage_cpu.py maps every recorded descriptor with point_class)."""
    return {c["cls"] for c in POINTWISE_CASES}


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _dev(t):
    return t.cuda()


def _assert_hi_nearest(hi, lo, name):
    """hi = fp16(the fp32 value) of an [hi | lo] pair: the pair stands for hi + lo, and hi is an fp16 nearest to it exactly when |lo| is at
    most half the spacing of the fp16 grid on lo's side of hi -- half a unit of hi's last place, or a quarter where hi is a power of two and
    lo points towards zero (the grid below a power of two is twice as fine).  (Comparing fp16(hi + lo) with hi instead would trip on values
    within 2^-12 of a midpoint, where lo rounds up to the half unit itself and the sum ties to even.)  The half unit is built from hi's
    exponent field as fp32 bits: 2^(field - 26), exact on any device."""
    bits = hi.contiguous().view(torch.int16).int()
    field = ((bits >> 10) & 31).clamp(min=1)
    half_ulp = ((field + 101) << 23).view(torch.float32)
    finer = ((bits & 0x3ff) == 0) & (((bits >> 10) & 31) > 1) & (torch.signbit(lo) != torch.signbit(hi)) & (lo != 0)
    limit = torch.where(finer, 0.5 * half_ulp, half_ulp)
    assert bool((lo.float().abs() <= limit).all()), f"{name}: hi is not fp16(hi + lo)"


def _flat_out(n, dtype, strided=True):
    """An output the C-ABI addresses as one dense run of n elements: guard rows of the same length in front and behind."""
    return lg.guarded(1, n, n + 64, dtype, pre_rows=1, post_rows=1, offset_cols=32 if strided else 0)


def _flat_in(t, post=64):
    return lg.poisoned(t.reshape(1, -1), ld=t.numel() + post, offset_cols=0).reshape(-1)


def _v1(ops, kind, **kw):
    ops.v1_op(kind, **kw)


# ======================================================================================================================================
# A. ops without a kernel-level test before this module
# ======================================================================================================================================
# ---- fill_rows: dst[img * rows_per_img + row_off, :D] = src[:D] ----
def _fill_make(c):
    return dict(src=_rnd((c["D"],), 1))


def _fill_eval(c, x, dt):
    return dict(dst=x["src"].to(dt).expand(c["n_img"], c["D"]).clone())


def _fill_bounds(c, x, ref):
    return dict(dst=torch.zeros(()))                                        # a copy: exact


def _fill_run(ops, c, x, strided):
    n, rpi, off, D = c["n_img"], c["rpi"], c["row_off"], c["D"]
    ld = D + (68 if strided else 0)
    rows = torch.arange(n) * rpi + off
    go = lg.guarded(n * rpi, D, ld, F32, offset_cols=4 if strided else 0, rows_inside=_dev(rows))
    src = _flat_in(_dev(x["src"]))
    ops.check(ops.lib.ud_fill_rows_f32(go.ptr(), src.data_ptr(), n, rpi, off, D, ld, ops.cur_stream()))
    return dict(dst=go.view[_dev(rows)]), [go]


OPS["fill_rows"] = Op(_fill_make, _fill_eval, _fill_bounds, _fill_run, dense=True)
_case("fill_rows", "vit_cls", (), n_img=3, rpi=37, row_off=0, D=384)         # the plans: (1, 1456, 0, 384 / 1024, ld = D)
_case("fill_rows", "row_off", (), n_img=2, rpi=9, row_off=5, D=1024)
_case("fill_rows", "D300", (), n_img=2, rpi=3, row_off=1, D=300)


# ---- V1 ADD: out = a + b over n fp32 values ----
def _add_make(c):
    return dict(a=_rnd((c["n"],), 1), b=_rnd((c["n"],), 2))


def _add_eval(c, x, dt):
    return dict(out=x["a"].to(dt) + x["b"].to(dt))


def _add_bounds(c, x, ref):
    return dict(out=lg.term_store_f32(ref["out"]))                          # one rounded addition


def _add_run(ops, c, x, strided):
    n = c["n"]
    go = _flat_out(n, F32)
    a, b = _flat_in(_dev(x["a"])), _flat_in(_dev(x["b"]))
    _v1(ops, K_ADD, a=a, b=b, out=go.view, i=(n & 0x7fffffff, n >> 31))
    return dict(out=go.view.reshape(-1)), [go]


OPS["add"] = Op(_add_make, _add_eval, _add_bounds, _add_run)
_case("add", "small", (), n=4 * 777)
_case("add", "second_trip", (), n=4 * (256 * 32 * 256 + 1000))                # grid1 caps the grid at 256 * 32 blocks: the stride loop runs twice


# ---- V1 MEAN3: out = (a + b + c) / 3 on column 0 of [n, ld] maps ----
def _mean3_make(c):
    return dict(a=_rnd((c["n"], 1), 1), b=_rnd((c["n"], 1), 2), c=_rnd((c["n"], 1), 3))


def _mean3_eval(c, x, dt):
    return dict(out=(x["a"].to(dt) + x["b"].to(dt) + x["c"].to(dt)) / 3)


def _mean3_bounds(c, x, ref):
    mag = (x["a"].double().abs() + x["b"].double().abs() + x["c"].double().abs()) / 3
    return dict(out=lg.term_rounding(mag, 3))


def _mean3_run(ops, c, x, strided):
    n, ld = c["n"], 4                                                        # the product's ld (depth maps are column 0 of 4-wide rows)
    ins = [lg.poisoned(_dev(x[k]), ld=ld, post_rows=8) for k in "abc"]
    go = lg.guarded(n, 1, ld, F32)                                           # columns 1..3 of every row are guard elements
    _v1(ops, K_MEAN3, a=ins[0], b=ins[1], c=ins[2], out=go.view, i=(n & 0x7fffffff, ld, n >> 31))
    return dict(out=go.view), [go]


OPS["mean3"] = Op(_mean3_make, _mean3_eval, _mean3_bounds, _mean3_run)
_case("mean3", "ld4", (), n=31 * 41)
_case("mean3", "second_trip", (), n=256 * 32 * 256 + 999)


# ---- V1 VIT_TAP: out = init ? v : max(out, v), v = patch tokens + class token; out2 = the raw class tokens ----
def _tap_make(c):
    B, Np, hw, D = c["B"], c["Np"], c["hw"], c["D"]
    x = _rnd((B, Np, D), 1)
    x[:, hw + 1:] = float("nan")                                             # pad rows past the image's tokens: poison
    return dict(x=x, prev=_rnd((B, hw, D), 2))


def _tap_eval(c, x, dt, no_cls=False):
    hw = c["hw"]
    t = x["x"].to(dt)
    v = t[:, 1:hw + 1] + (0 if no_cls else t[:, :1])
    out = dict(smax=v if c["init"] else torch.maximum(x["prev"].to(dt), v))
    if c["out2"]:
        out["cls"] = t[:, 0].clone()
    return out


def _tap_bounds(c, x, ref):
    t = x["x"].double()
    v = t[:, 1:c["hw"] + 1].abs() + t[:, :1].abs()
    b = dict(smax=lg.term_store_f32(v))                                      # one rounded addition; the maximum selects
    if c["out2"]:
        b["cls"] = torch.zeros(())
    return b


def _tap_run(ops, c, x, strided):
    B, Np, hw, D = c["B"], c["Np"], c["hw"], c["D"]
    xin = _flat_in(_dev(x["x"]))
    go = lg.guarded(B * hw, D, D, F32, init=_dev(x["prev"]).reshape(B * hw, D) if not c["init"] else None)
    gs, out = [go], dict(smax=go.view.view(B, hw, D))
    cls = None
    if c["out2"]:
        gc = lg.guarded(B, D, D, F32)
        gs.append(gc)
        cls, out["cls"] = gc.view, gc.view
    _v1(ops, K_VIT_TAP, a=xin, out=go.view, out2=cls, i=(B, Np, hw, D, c["init"]))
    return out, gs


OPS["vit_tap"] = Op(_tap_make, _tap_eval, _tap_bounds, _tap_run)
for _init, _o2 in ((1, 0), (0, 0), (0, 1), (1, 1)):                           # the plan: (1, 1456, 1452, 1024, init 0 / 1), out2 with init 0
    _case("vit_tap", f"init{_init}_cls{_o2}", (_init, _o2), B=2, Np=50, hw=45, D=1024, init=_init, out2=_o2)
_case("vit_tap", "second_trip", (0, 1), B=1, Np=2110, hw=2101, D=1024, init=0, out2=1)      # the grid is capped at 2048 blocks per image


# ---- V1 COPY_ROWS ----
def _copy_make(c):
    return dict(src=_rnd((c["n_img"] * c["T"], c["D"]), 1))


def _copy_eval(c, x, dt, drop_lo=False):
    s = x["src"]
    if c["to_f16"] == 0:
        return dict(out=s.to(dt))
    if c["to_f16"] == 1:
        return dict(out=s.to(dt))
    hi = s.half()
    return dict(hi=hi, total=hi.to(dt) if drop_lo else s.to(dt))              # total: the value the two terms stand for


def _copy_bounds(c, x, ref):
    if c["to_f16"] < 2:
        return dict(out=torch.zeros(()))                                      # a copy, or a conversion: nothing but the store
    return dict(hi=torch.zeros(()), total=torch.zeros(()))                    # hi = fp16(x) exactly


def _copy_run(ops, c, x, strided):
    n, T, rpi, off, D, mode = c["n_img"], c["T"], c["rpi"], c["row_off"], c["D"], c["to_f16"]
    w = 2 * D if mode == 2 else D
    dt = F32 if mode == 0 else F16
    ld = w + (72 if strided else 0)
    rows = (torch.arange(n)[:, None] * rpi + off + torch.arange(T)[None]).reshape(-1)
    go = lg.guarded(n * rpi, w, ld, dt, offset_cols=8 if strided else 0, rows_inside=_dev(rows))
    src = _flat_in(_dev(x["src"]))
    _v1(ops, K_COPY_ROWS, a=src, out=go.view, i=(n, T, rpi, off, D, ld, mode))
    got = go.view[_dev(rows)]
    if mode == 2:
        _assert_hi_nearest(got[:, :D], got[:, D:], c["id"])
        return dict(hi=got[:, :D], total=got[:, :D].double() + got[:, D:].double()), [go]
    return dict(out=got), [go]


OPS["copy_rows"] = Op(_copy_make, _copy_eval, _copy_bounds, _copy_run, dense=True, stores=lambda c: {0: {}, 1: dict(out="f16"), 2: dict(total="pair")}[c["to_f16"]])
_case("copy_rows", "f32_row_off", (0, True), n_img=2, T=4, rpi=49, row_off=45, D=512, to_f16=0)     # the plan: (1, 4, 4260, 4256, 512, 512, 0)
_case("copy_rows", "f16_row_off", (1, True), n_img=2, T=4, rpi=49, row_off=45, D=512, to_f16=1)
_case("copy_rows", "f16", (1, False), n_img=3, T=21, rpi=21, row_off=0, D=100, to_f16=1)
_case("copy_rows", "split", (2, False), n_img=1, T=133, rpi=133, row_off=0, D=128, to_f16=2)        # the plan: (1, hw, hw, 0, 128 / 256 / 512, 2 D, 2)
_case("copy_rows", "split_row_off", (2, True), n_img=2, T=17, rpi=25, row_off=3, D=512, to_f16=2)
_case("copy_rows", "f32", (0, False), n_img=2, T=5, rpi=5, row_off=0, D=64, to_f16=0)
_case("copy_rows", "second_trip", (2, False), n_img=1, T=8300, rpi=8300, row_off=0, D=256, to_f16=2)


# ---- camera tails: V1 CAMERA and ud_camera_intrinsics ----
# T_CAM: unit 2^-24 x the entry's expression on absolute values; torch fp32 of the exp / sigmoid chains against fp64 on these cases: 4.05
T_CAM = 17.0


def _cam_make(c):
    return dict(raw=_rnd((c["B"], 4), 5, 0.7))


def _cam_terms(c, raw, dt, mag=False):
    """(fx, fy, cx, cy) and the derived matrices; mag: every difference / quotient on absolute values."""
    Hn, Wn = c["Hn"], c["Wn"]
    o = raw.to(dt)
    if c["op"] == "camera_v1":
        s = torch.tensor(0.5 * max(Hn, Wn), dtype=dt)
    else:
        s = torch.sqrt(torch.tensor(float(Hn * Hn + Wn * Wn), dtype=dt)) * torch.tensor(0.7, dtype=F32).to(dt)
    fx, fy = torch.exp(o[:, 0]) * s, torch.exp(o[:, 1]) * s
    cx, cy = torch.sigmoid(o[:, 2]) * Wn, torch.sigmoid(o[:, 3]) * Hn
    z, one = torch.zeros_like(fx), torch.ones_like(fx)
    sg = 1.0 if mag else -1.0
    K = torch.stack([fx, z, cx, z, fy, cy, z, z, one], 1)
    Ki = torch.stack([1 / fx, z, sg * cx / fx, z, 1 / fy, sg * cy / fy, z, z, one], 1)
    pl, pt = c["pad_l"], c["pad_t"]
    r = torch.tensor(c["ratio"], dtype=F32).to(dt)
    if c["op"] == "camera_v1":
        Kp = torch.stack([fx / r, z, (cx + sg * pl) / r, z, fy / r, (cy + sg * pt) / r, z, z, one], 1)
    else:
        Kp = torch.stack([fx / r, z, cx / r + sg * pl, z, fy / r, cy / r + sg * pt, z, z, one], 1)
    out = dict(K=K, Kinv=Ki, Kpost=Kp)
    if c["op"] == "camera_intrinsics":
        out["intr4"] = torch.stack([fx, fy, cx, cy], 1)
    return out


def _cam_eval(c, x, dt):
    return _cam_terms(c, x["raw"], dt)


def _cam_bounds(c, x, ref):
    return {k: T_CAM * U24 * v for k, v in _cam_terms(c, x["raw"], F64, mag=True).items()}


def _cam_run(ops, c, x, strided):
    B = c["B"]
    gs = {k: lg.guarded(B, 9, 9, F32) for k in ("K", "Kinv", "Kpost")}
    if c["op"] == "camera_v1":
        raw = _flat_in(_dev(x["raw"]))
        _v1(ops, K_CAMERA, a=raw, out=gs["K"].view, out2=gs["Kinv"].view, c=gs["Kpost"].view, i=(B, c["Hn"], c["Wn"], c["pad_l"], c["pad_t"]), f=(c["ratio"],))
    else:
        st = c["raw_stride"]
        raw = lg.poisoned(_dev(x["raw"]).reshape(B * 4, 1), ld=st, post_rows=4)          # the parameters sit `raw_stride` floats apart
        gs["intr4"] = lg.guarded(B, 4, 4, F32)
        ops.check(ops.lib.ud_camera_intrinsics(raw.data_ptr(), st, gs["intr4"].ptr(), gs["K"].ptr(), gs["Kinv"].ptr(), gs["Kpost"].ptr(), B, c["Hn"], c["Wn"],
                                               c["ratio"], c["pad_l"], c["pad_t"], ops.cur_stream()))
    return {k: g.view for k, g in gs.items()}, list(gs.values())


OPS["camera_v1"] = Op(_cam_make, _cam_eval, _cam_bounds, _cam_run)
OPS["camera_intrinsics"] = Op(_cam_make, _cam_eval, _cam_bounds, _cam_run)
_case("camera_v1", "plan", (), B=3, Hn=462, Wn=616, pad_l=0, pad_t=0, ratio=1.925)      # the plan: (1, 462, 616, 0, 0), f = 1.925
_case("camera_v1", "padded", (), B=70, Hn=616, Wn=462, pad_l=7, pad_t=21, ratio=0.75)   # B > 64: a second block
_case("camera_intrinsics", "stride1", (False,), B=3, Hn=462, Wn=616, pad_l=0, pad_t=0, ratio=1.0, raw_stride=1)
_case("camera_intrinsics", "stride5", (True,), B=66, Hn=322, Wn=518, pad_l=13, pad_t=4, ratio=1.3125, raw_stride=5)


# ---- ud_rays_from_kinv, gt_mode 0..3 ----
# T_SPH: unit 2^-24 (absolute, the rays are unit vectors); torch fp32 of the Spherical statement against fp64 on this case: 2.08
T_SPH = 9.0


def _restate():
    from oracle import restate
    return restate.OracleV2


@contextlib.contextmanager
def _default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _rays_make(c):
    nb, Hn, Wn, mode = c["nb"], c["Hn"], c["Wn"], c["gt_mode"]
    g = torch.Generator().manual_seed(7)
    p = torch.zeros(nb, 9)
    if mode in (0, 1):                                                       # a general inverse intrinsic matrix: every entry matters
        f = 0.6 * math.hypot(Hn, Wn) * (1 + 0.2 * torch.rand(nb, generator=g))
        p[:, 0], p[:, 4] = 1 / f, 1.1 / f
        p[:, 2], p[:, 5] = -0.5 * Wn / f, -0.45 * Hn / f
        p[:, 1], p[:, 3] = 0.01 / f, -0.02 / f
        p[:, 6], p[:, 7], p[:, 8] = 1e-4 * torch.randn(nb, generator=g), 1e-4 * torch.randn(nb, generator=g), 1.0
    elif mode == 2:
        # EUCM (fx, fy, cx, cy, alpha, beta); dyadic values: oracle/restate.py combines the parameters as fp32 scalars before they meet
        # the fp64 grid, and with these every such product is exact
        for b in range(nb):
            p[b, :6] = torch.tensor([160.0 + 32 * b, 176.0, 0.5 * Wn + 4 * b, 0.5 * Hn - 2, 0.625, 1.25])
    else:
        for b in range(nb):                                                  # Spherical (fx, fy, cx, cy, width, height, hfov / 2, vfov / 2)
            p[b, :8] = torch.tensor([1.0, 1.0, 0.0, 0.0, float(Wn + 2 * b), float(Hn), 1.5 - 0.25 * b, 0.75])
    return dict(p=p)


def _rays_eval(c, x, dt):
    nb, Hn, Wn, mode = c["nb"], c["Hn"], c["Wn"], c["gt_mode"]
    p = x["p"]
    if mode >= 2:
        with _default_dtype(dt):                                             # oracle/restate.py's camera restatement, evaluated at `dt`
            r = torch.cat([_restate()._rays_from_camera_model("EUCM" if mode == 2 else "Spherical", p[b], (0, 0, 0, 0), 1.0, Hn, Wn) for b in range(nb)])
        return dict(rays=r.to(dt))
    k = p.to(dt)
    u = (torch.arange(Wn, dtype=dt) + 0.5).view(1, 1, Wn)
    v = (torch.arange(Hn, dtype=dt) + 0.5).view(1, Hn, 1)
    kk = [k[:, i].view(nb, 1, 1) for i in range(9)]
    xyz = torch.stack([kk[0] * u + kk[1] * v + kk[2], kk[3] * u + kk[4] * v + kk[5], kk[6] * u + kk[7] * v + kk[8]], 1)
    if mode == 1:
        xyz = xyz / xyz[:, 2:3].clamp(min=1e-4)
    return dict(rays=xyz / torch.norm(xyz, dim=1, keepdim=True).clamp(min=1e-4 if mode == 1 else 1e-5))


def _rays_bounds(c, x, ref):
    nb, Hn, Wn, mode = c["nb"], c["Hn"], c["Wn"], c["gt_mode"]
    if mode == 3:
        return dict(rays=torch.full((), T_SPH * U24, dtype=F64))
    p = x["p"].double()
    u = (torch.arange(Wn, dtype=F64) + 0.5).view(1, 1, Wn)
    v = (torch.arange(Hn, dtype=F64) + 0.5).view(1, Hn, 1)
    a = [p[:, i].abs().view(nb, 1, 1) for i in range(9)]
    if mode == 2:                                                            # m = (pixel - c) / f, mz from r^2: magnitudes of the unnormalised direction
        mx, my = (u + a[2]) / a[0], (v + a[3]) / a[1]
        mags = [mx.expand(nb, Hn, Wn), my.expand(nb, Hn, Wn), (1.0 + mx * mx + my * my).expand(nb, Hn, Wn)]
        nrm = torch.ones(())                                                 # |(mx, my, mz)| >= ~1 / (1 + ...): the restatement normalises by cf first
        taps = 16
    else:
        mags = [a[0] * u + a[1] * v + a[2], a[3] * u + a[4] * v + a[5], a[6] * u + a[7] * v + a[8]]
        kk = [p[:, i].view(nb, 1, 1) for i in range(9)]
        xyz = torch.stack([kk[0] * u + kk[1] * v + kk[2], kk[3] * u + kk[4] * v + kk[5], kk[6] * u + kk[7] * v + kk[8]], 1)
        nrm = torch.norm(xyz / (xyz[:, 2:3] if mode == 1 else 1.0), dim=1).clamp(min=1e-4)
        if mode == 1:
            mags = [m / xyz[:, 2].abs() for m in mags]
        taps = 3
    # a component's error moves every normalised component: 2 max_j d_j / |u|, plus the rounding of the unit-length result itself
    e = torch.stack([lg.term_rounding(m, taps) for m in mags], 1).amax(1, keepdim=True)
    return dict(rays=(2 * e / (nrm if nrm.dim() == 0 else nrm.unsqueeze(1)) + 4 * U24).expand(nb, 3, Hn, Wn))


def _rays_run(ops, c, x, strided):
    nb, Hn, Wn = c["nb"], c["Hn"], c["Wn"]
    p = lg.poisoned(_dev(x["p"]), post_rows=2)
    go = _flat_out(nb * 3 * Hn * Wn, F32)
    ops.check(ops.lib.ud_rays_from_kinv(p.data_ptr(), go.ptr(), nb, Hn, Wn, c["gt_mode"], ops.cur_stream()))
    return dict(rays=go.view.view(nb, 3, Hn, Wn)), [go]


OPS["rays"] = Op(_rays_make, _rays_eval, _rays_bounds, _rays_run)
for _m in range(4):
    _case("rays", f"mode{_m}", (_m,), nb=2, Hn=42, Wn=56, gt_mode=_m)        # the plans: (1, 462, 616, 0)
_case("rays", "second_trip", (0,), nb=1, Hn=520, Wn=523, gt_mode=0)           # more than 1024 blocks of 256 pixels


# ---- ud_max_f32, ud_spatial_mean_f32 ----
def _max_make(c):
    return dict(dst=_rnd((c["n"],), 1), src=_rnd((c["n"],), 2))


def _max_eval(c, x, dt):
    return dict(dst=x["src"].to(dt) if c["init"] else torch.maximum(x["dst"].to(dt), x["src"].to(dt)))


def _max_bounds(c, x, ref):
    return dict(dst=torch.zeros(()))


def _max_run(ops, c, x, strided):
    n = c["n"]
    go = _flat_out(n, F32)
    if not c["init"]:
        go.view.copy_(_dev(x["dst"]).view(1, n))
    src = _flat_in(_dev(x["src"]))
    ops.check(ops.lib.ud_max_f32(go.ptr(), src.data_ptr(), n, c["init"], ops.cur_stream()))
    return dict(dst=go.view.reshape(-1)), [go]


OPS["max"] = Op(_max_make, _max_eval, _max_bounds, _max_run)
_case("max", "init", (1,), n=4 * 1111, init=1)
_case("max", "running", (0,), n=4 * 1111, init=0)
_case("max", "second_trip", (0,), n=4 * (256 * 16 * 256 + 77), init=0)


def _smean_make(c):
    return dict(x=_rnd((c["B"], c["HW"], c["C"]), 1) + 0.3)


def _smean_eval(c, x, dt, hw_plus_one=False):
    return dict(out=x["x"].to(dt).sum(1) / (c["HW"] + (1 if hw_plus_one else 0)))


def _smean_bounds(c, x, ref):
    return dict(out=lg.term_rounding(x["x"].double().abs().mean(1), c["HW"]))


def _smean_run(ops, c, x, strided):
    B, HW, Cc = c["B"], c["HW"], c["C"]
    ldo = Cc + (132 if strided else 0)
    go = lg.guarded(B, Cc, ldo, F32, offset_cols=4 if strided else 0)
    xin = _flat_in(_dev(x["x"]))
    ops.check(ops.lib.ud_spatial_mean_f32(xin.data_ptr(), go.ptr(), B, HW, Cc, ldo, ops.cur_stream()))
    return dict(out=go.view), [go]


OPS["spatial_mean"] = Op(_smean_make, _smean_eval, _smean_bounds, _smean_run, dense=True)
_case("spatial_mean", "C768", (True,), B=2, HW=133, C=768)                    # the plan: (1, 1064, 768, 768), (1, 266, 1536, 1536)
_case("spatial_mean", "C1536", (True,), B=3, HW=35, C=1536)
_case("spatial_mean", "C100", (False,), B=2, HW=7, C=100)


# ======================================================================================================================================
# B. resampling
# ======================================================================================================================================
def _axis(n_out, n_in, dt, align_corners, scale=None, half_pixel=True, clamp=True):
    """Source indices and weight of one axis of a bilinear resize, computed at `dt` the way the kernels compute them."""
    o = torch.arange(n_out, dtype=dt)
    if align_corners:
        s = (torch.tensor(n_in - 1, dtype=dt) / torch.tensor(n_out - 1, dtype=dt)) if n_out > 1 else torch.tensor(0.0, dtype=dt)
        f = s * o
    else:
        s = torch.tensor(scale, dtype=dt) if scale is not None else torch.tensor(n_in, dtype=dt) / torch.tensor(n_out, dtype=dt)
        f = (s * (o + 0.5) - 0.5) if half_pixel else s * o
        f = f.clamp(min=0)
    i0 = f.floor().long().clamp(max=n_in - 1)
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0) if clamp else (i0 + 1) % n_in   # clamp omitted: the border tap reads the wrapped-around neighbour
    return i0, i1, f - i0.to(dt)


def _bilinear(x, Ho, Wo, dt, align_corners, scale=None, half_pixel=True, clamp=True, swap_rows=False, absval=False, taps=False):
    """Bilinear resize of NHWC `x` [B, H, W, C]; absval: on absolute values (mag); taps: the plain sum of the four |tap values|."""
    B, H, W, Cc = x.shape
    v = x.to(dt)
    if absval or taps:
        v = v.abs()
    y0, y1, ly = _axis(Ho, H, dt, align_corners, scale, half_pixel, clamp)
    x0, x1, lx = _axis(Wo, W, dt, align_corners, scale, half_pixel, clamp)
    if swap_rows:
        ly = torch.where(ly > 0, 1 - ly, ly)
    ly, lx = ly.view(1, Ho, 1, 1), lx.view(1, 1, Wo, 1)
    r0, r1 = v[:, y0], v[:, y1]
    v00, v01, v10, v11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    if taps:
        return v00 + v01 + v10 + v11
    return (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)


def _axis_weights(kind, n_out, n_in):
    """(W, S) of _axis_at with S widened to every tap the axis can read when its fp32 source coordinate is off by a rounding: where a coordinate
    falls on an integer (or a filter edge on a sample), the fp32 one may land on the other side and read the next tap with a weight of ~0,
    and the result then moves by delta x that tap's difference to its neighbour."""
    W, S = _axis_at(kind, n_out, n_in, 0.0)
    return W, torch.maximum(S, torch.maximum(_axis_at(kind, n_out, n_in, -2.0 ** -10)[1], _axis_at(kind, n_out, n_in, 2.0 ** -10)[1]))


def _axis_at(kind, n_out, n_in, shift):
    """One axis of a separable resize as explicit fp64 matrices [n_out, n_in]: (W, S), W the interpolation weights and S the 0 / 1 support
    (the taps the axis reads).  kind "aa": the antialiased triangle filter of support max(scale, 1), normalised to sum 1 (ATen's
    _upsample_bilinear2d_aa); "linear": bilinear, align_corners=False; "cubic": bicubic with A = -0.75, un-clamped coordinate, border-clamped
    taps (a clamped tap's weight lands on the border sample).  shift: added to every source coordinate."""
    o = torch.arange(n_out, dtype=F64)
    j = torch.arange(n_in, dtype=F64)
    s = n_in / n_out
    if kind == "aa":
        sup, c = max(s, 1.0), s * (o + 0.5) + shift
        lo, hi = (c - sup + 0.5).floor().clamp(min=0), (c + sup + 0.5).floor().clamp(max=n_in)
        S = ((j[None] >= lo[:, None]) & (j[None] < hi[:, None])).double()
        W = (1 - ((j[None] - c[:, None] + 0.5) / sup).abs()).clamp(min=0) * S
        return W / W.sum(1, keepdim=True), S
    W = torch.zeros(n_out, n_in, dtype=F64)
    f = s * (o + 0.5) - 0.5 + shift
    if kind == "linear":
        f = f.clamp(min=0)
        i0 = f.floor().long().clamp(max=n_in - 1)
        taps = ((i0, 1 - (f - i0)), ((i0 + 1).clamp(max=n_in - 1), f - i0))
    else:
        A, i0 = -0.75, f.floor().long()
        t = f - i0

        def inner(d):
            return ((A + 2) * d - (A + 3)) * d * d + 1

        def outer(d):
            return ((A * d - 5 * A) * d + 8 * A) * d - 4 * A
        taps = tuple(((i0 - 1 + k).clamp(0, n_in - 1), w) for k, w in enumerate((outer(t + 1), inner(t), inner(1 - t), outer(2 - t))))
    S = torch.zeros_like(W)
    rows = torch.arange(n_out)
    for idx, w in taps:
        W.index_put_((rows, idx), w, accumulate=True)
        S[rows, idx] = 1.0
    return W, S


def _separable(t, My, Mx):
    """My t Mx^T over the last two axes of t [..., H, W]."""
    return torch.einsum("oh,...hw,pw->...op", My, t.double(), Mx)


def _separable_bound(t, wy, wx):
    """Rounding and source-coordinate terms of a separable resize of t [..., H, W] with the axes' (W, S) pairs: mag is the resize on absolute
    values with absolute weights, and the coordinate term (max source coordinate) 2^-22 x the sum of the |tap values| the element reads."""
    (Wy, Sy), (Wx, Sx) = wy, wx
    a = t.double().abs()
    taps = int(Sy.sum(1).max() * Sx.sum(1).max())
    return lg.term_rounding(_separable(a, Wy.abs(), Wx.abs()), taps) + lg.term_coord(max(Wy.shape[1], Wx.shape[1]), _separable(a, Sy, Sx))


def _ln(v, eps):
    m = v.mean(-1, keepdim=True)
    d = v - m
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)


def _ln_bound(v64, e_in, eps):
    """Bound of y = (v - mean) rsqrt(var + eps) over the last axis when every v carries an error <= e_in (tensor or 0): with e = max e_in +
    the fp32 rounding of the mean / centred values (C terms), |dy| <= 2 e rstd (1 + |y|) -- d(v - mean) <= 2 e, d var <= 2 sqrt(var) 2 e
    (Cauchy-Schwarz), so d rstd / rstd <= 2 e sqrt(var) / (var + eps) <= 2 e rstd -- plus the rounding of the product."""
    Cc = v64.shape[-1]
    m = v64.mean(-1, keepdim=True)
    d = v64 - m
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    y = d * rstd
    e = (e_in.amax(-1, keepdim=True) if isinstance(e_in, torch.Tensor) and e_in.dim() else e_in) + lg.term_rounding(v64.abs().amax(-1, keepdim=True), Cc)
    return 2 * e * rstd * (1 + y.abs()) + 4 * U24 * y.abs()


def _lowvar(x, eps, rows):
    """Scale `rows` (a slice of the leading axes) so their standard deviation is ~10 sqrt(eps): a wrong or dropped eps moves them by 4 %."""
    x[rows] = x[rows] * (10.0 * math.sqrt(eps))
    return x


# ---- ud_upsample2x_nhwc ----
def _up_path(mode, Cc, ldy):
    """The kernel ud_upsample2x_nhwc dispatches to (pointwise.hip)."""
    if mode == 0:
        return "f32"
    g8 = Cc >> 3
    if Cc % 8 == 0 and (g8 & (g8 - 1)) == 0 and g8 <= 64 and ldy % 8 == 0:
        return "ln8"
    g = Cc >> 2
    return "shuffle" if (g & (g - 1)) == 0 and g <= 64 else ("lds" if g <= 64 else "lds_wide")


def _up_ld(c, strided):
    Cc = c["C"]
    if not strided:
        return Cc, Cc, 0, 0
    ldy = Cc + c.get("ypad", 24)
    return Cc + 20, ldy, 4, c.get("yoff", 8 if c["mode"] else 4)


def _up_make(c):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    x = _rnd((B, H, W, Cc), 1) + 0.2
    if c["mode"] == 1:
        _lowvar(x, c["eps"], (B - 1, slice(H // 2, H)))                      # the lower half of the last image
    return dict(x=x)


def _up_eval(c, x, dt, eps_scale=1.0, **defect):
    v = _bilinear(x["x"], 2 * c["H"], 2 * c["W"], dt, False, scale=0.5, **defect)
    if c["mode"] == 1:
        v = _ln(v, c["eps"] * eps_scale)
    return dict(out=v)


def _up_bounds(c, x, ref):
    # source coordinates 0.5 (o + 0.5) - 0.5 are multiples of 1/4 below 2^22: exact in fp32, so no coordinate term
    e = lg.term_rounding(_bilinear(x["x"], 2 * c["H"], 2 * c["W"], F64, False, scale=0.5, absval=True), 4)
    if c["mode"] == 0:
        return dict(out=e)
    return dict(out=_ln_bound(_bilinear(x["x"], 2 * c["H"], 2 * c["W"], F64, False, scale=0.5), e, c["eps"]))


def _up_run(ops, c, x, strided):
    B, H, W, Cc, mode = c["B"], c["H"], c["W"], c["C"], c["mode"]
    ldin, ldy, ioff, yoff = _up_ld(c, strided)
    rows_img = H * W + (c.get("in_pad", 0) if strided or c.get("in_pad_dense") else 0)
    xin = torch.full((B, rows_img, Cc), float("nan"))
    xin[:, :H * W] = x["x"].reshape(B, H * W, Cc)                             # rows past H * W of an image: poison
    X = lg.poisoned(_dev(xin).reshape(B * rows_img, Cc), ld=ldin, offset_cols=ioff, post_rows=4)
    go = lg.guarded(B * 4 * H * W, Cc, ldy, F16 if mode else F32, offset_cols=yoff)
    assert _up_path(mode, Cc, ldy) == c["cls"][2] or not strided, (c["id"], _up_path(mode, Cc, ldy))
    d = ops.mk(ops.UdUpsample2x, in_=X, out=go.view, B=B, H=H, W=W, C=Cc, ldin=ldin, ldy=ldy, mode=mode, eps=c.get("eps", 0.0), in_img_rows=rows_img if rows_img != H * W else 0)
    ops.check(ops.lib.ud_upsample2x_nhwc(C.byref(d), ops.cur_stream()))
    return dict(out=go.view.view(B, 2 * H, 2 * W, Cc)), [go]


OPS["upsample2x"] = Op(_up_make, _up_eval, _up_bounds, _up_run, dense=True, stores=lambda c: dict(out="f16") if c["mode"] else {})
# the plans: mode 1, C = 64 / 128, ld = C, in_img_rows = H W (ln8).  ypad / yoff pick the kernel: ldy % 8 == 4 leaves ln8 for the generic one
_case("upsample2x", "ln8_C64", (1, "ln8"), B=2, H=9, W=11, C=64, mode=1, eps=1e-5, in_pad=5)
_case("upsample2x", "ln8_C128", (1, "ln8"), B=2, H=7, W=13, C=128, mode=1, eps=1e-5, in_pad=3)
# (dense=False: at ldy = C these shapes run the ln8 kernel, whose statistics are summed in another order -- no bit-identity to ask for)
_case("upsample2x", "shuffle_C64", (1, "shuffle"), B=2, H=9, W=11, C=64, mode=1, eps=1e-5, in_pad=5, ypad=28, yoff=4, dense=False)
_case("upsample2x", "shuffle_C256", (1, "shuffle"), B=2, H=5, W=7, C=256, mode=1, eps=1e-5, ypad=12, yoff=4, dense=False)
_case("upsample2x", "lds_C96", (1, "lds"), B=2, H=9, W=11, C=96, mode=1, eps=1e-5, in_pad=2)
_case("upsample2x", "lds_C512", (1, "lds_wide"), B=2, H=5, W=7, C=512, mode=1, eps=1e-5, in_pad=1, ypad=20, yoff=4, dense=False)
_case("upsample2x", "f32_C64", (0, "f32"), B=2, H=9, W=11, C=64, mode=0, in_pad=5)
_case("upsample2x", "f32_C96", (0, "f32"), B=2, H=6, W=5, C=96, mode=0)
_case("upsample2x", "f32_C512", (0, "f32"), B=1, H=5, W=7, C=512, mode=0, in_pad=2)
_case("upsample2x", "f32_second_trip", (0, "f32"), B=2, H=16400, W=2, C=4, mode=0)      # 2 B H > 65535 rows of the grid
_case("upsample2x", "ln8_second_trip", (1, "ln8"), B=2, H=32800, W=1, C=8, mode=1, eps=1e-5)   # B (H + 1) > 65535 row pairs
# the generic mode-1 kernel shares the row-capped grid of mode 0: its shuffle path (ldy % 8 == 4) and its LDS path (barriers inside the row loop)
_case("upsample2x", "shuffle_second_trip", (1, "shuffle"), B=2, H=16400, W=2, C=4, mode=1, eps=1e-5, ypad=8, yoff=4)
_case("upsample2x", "lds_second_trip", (1, "lds"), B=2, H=16400, W=2, C=12, mode=1, eps=1e-5, ypad=8, yoff=4)


# ---- ud_resize_ac_nhwc_f16 and V1 RESIZE_AC_SPLIT (align_corners=True) ----
def _ac_make(c):
    if "second_trip" in c["id"]:
        # over ~10^7 elements the extreme of |v1 - v0| / sum |taps| reaches the coordinate term's worst case, where two fp32 roundings of the
        # coordinate (2^-23) leave only a factor 2 under the term (2^-22): the maps that only exist to run the stride loop twice carry an offset
        x = _rnd((c["G"] * c["B"] if c["op"] == "resize_ac" else c["B"], c["Hin"], c["Win"], c["C"]), 1, 0.25) + 1.0
        return dict(x=x.half() if c["op"] == "resize_ac" else x)
    return dict(x=_rnd((c["G"] * c["B"], c["Hin"], c["Win"], c["C"]), 1).half() if c["op"] == "resize_ac" else _rnd((c["B"], c["Hin"], c["Win"], c["C"]), 1))


def _ac_eval(c, x, dt, flip_align=False, drop_lo=False):
    v = _bilinear(x["x"], c["Hout"], c["Wout"], dt, not flip_align)
    if c["op"] == "resize_ac":
        return dict(out=v)
    return dict(total=v.half().to(dt) if drop_lo else v)


def _ac_bounds(c, x, ref):
    e = lg.term_rounding(_bilinear(x["x"], c["Hout"], c["Wout"], F64, True, absval=True), 4) + \
        lg.term_coord(max(c["Hin"], c["Win"]), _bilinear(x["x"], c["Hout"], c["Wout"], F64, True, taps=True))
    return dict(out=e) if c["op"] == "resize_ac" else dict(total=e)


def _ac_run(ops, c, x, strided):
    B, Cc, Hi, Wi, Ho, Wo = c["B"], c["C"], c["Hin"], c["Win"], c["Hout"], c["Wout"]
    xin = _flat_in(_dev(x["x"]))
    if c["op"] == "resize_ac":
        G = c["G"]
        go = _flat_out(G * B * Ho * Wo * Cc, F16)
        d = ops.mk(ops.UdResizeAC, in_=xin, out=go.view, G=G, B=B, Hin=Hi, Win=Wi, Hout=Ho, Wout=Wo, C=Cc)
        ops.check(ops.lib.ud_resize_ac_nhwc_f16(C.byref(d), ops.cur_stream()))
        return dict(out=go.view.view(G * B, Ho, Wo, Cc)), [go]
    go = _flat_out(B * Ho * Wo * 2 * Cc, F16)
    _v1(ops, K_RESIZE_AC_SPLIT, a=xin, out=go.view, i=(B, Hi, Wi, Ho, Wo, Cc))
    o = go.view.view(B, Ho, Wo, 2, Cc)
    hi, lo = o[..., 0, :], o[..., 1, :]
    _assert_hi_nearest(hi, lo, c["id"])
    return dict(total=hi.double() + lo.double()), [go]


OPS["resize_ac"] = Op(_ac_make, _ac_eval, _ac_bounds, _ac_run, stores=lambda c: dict(out="f16"))
OPS["resize_ac_split"] = Op(_ac_make, _ac_eval, _ac_bounds, _ac_run, stores=lambda c: dict(total="pair"))
_case("resize_ac", "G2", (True,), G=2, B=2, Hin=24, Win=32, Hout=42, Wout=56, C=32)     # the plan: G 2, 264 x 352 -> 462 x 616, C 32
_case("resize_ac", "G1_down", (False,), G=1, B=1, Hin=21, Win=17, Hout=9, Wout=8, C=8)
_case("resize_ac", "second_trip", (True,), G=2, B=1, Hin=3, Win=3, Hout=33000, Wout=2, C=8)     # G B Hout > 65535 grid rows
for _cc, _hw in ((64, (14, 19)), (128, (7, 10)), (256, (5, 7))):               # the plans: x2 at C = 64 / 128 / 256
    _case("resize_ac_split", f"C{_cc}", (_cc,), B=2, Hin=_hw[0], Win=_hw[1], Hout=2 * _hw[0], Wout=2 * _hw[1], C=_cc)
_case("resize_ac_split", "second_trip", (64,), B=1, Hin=130, Win=140, Hout=260, Wout=520, C=64)  # more than 256 * 32 * 256 (pixel, 4 channels) items


# ---- V1 RESIZE_AA: antialiased bilinear resize of a crop window ----
def _aa_make(c):
    if "second_trip" in c["id"]:                                              # see _ac_make: ~10^7 elements reach the coordinate term's worst case
        return dict(x=_rnd((c["B"], c["Hi"], c["Wi"], c["C"]), 1, 0.25) + 1.0)
    return dict(x=_rnd((c["B"], c["Hi"], c["Wi"], c["C"]), 1))


def _aa_win(c, x, dt):
    return x["x"][:, c["y0"]:c["y0"] + c["Hc"], c["x0"]:c["x0"] + c["Wc"]].to(dt).permute(0, 3, 1, 2)


def _aa_eval(c, x, dt, no_antialias=False, tap=None):
    if tap:                                                                   # planted: the first support tap of every output row 1 % heavy, or missing
        (Wy, _), (Wx, _) = _axis_weights("aa", c["Ho"], c["Hc"]), _axis_weights("aa", c["Wo"], c["Wc"])
        rows, first = torch.arange(c["Ho"]), (Wy > 0).double().argmax(1)
        Wy[rows, first] *= 1.01 if tap == "heavy" else 0.0
        Wy = Wy / Wy.sum(1, keepdim=True) if tap == "missing" else Wy
        return dict(out=_separable(_aa_win(c, x, F64), Wy, Wx).permute(0, 2, 3, 1).to(dt))
    v = F.interpolate(_aa_win(c, x, dt), size=(c["Ho"], c["Wo"]), mode="bilinear", align_corners=False, antialias=not no_antialias)
    return dict(out=v.permute(0, 2, 3, 1))


def _aa_bounds(c, x, ref):
    e = _separable_bound(_aa_win(c, x, F64), _axis_weights("aa", c["Ho"], c["Hc"]), _axis_weights("aa", c["Wo"], c["Wc"]))
    return dict(out=e.permute(0, 2, 3, 1))


def _aa_run(ops, c, x, strided):
    B, Hi, Wi, Ho, Wo, Cc = c["B"], c["Hi"], c["Wi"], c["Ho"], c["Wo"], c["C"]
    ldi, ldo = (Cc + 12, Cc + 36) if strided else (Cc, Cc)
    X = lg.poisoned(_dev(x["x"]).reshape(B * Hi * Wi, Cc), ld=ldi, offset_cols=4 if strided else 0, post_rows=2)
    go = lg.guarded(B * Ho * Wo, Cc, ldo, F32, offset_cols=8 if strided else 0)
    _v1(ops, K_RESIZE_AA, a=X, out=go.view, i=(B, Hi, Wi, Ho, Wo, Cc, ldi, ldo, c["y0"], c["x0"], c["Hc"], c["Wc"]))
    return dict(out=go.view.view(B, Ho, Wo, Cc)), [go]


def _aa_case(id, B, Hi, Wi, Ho, Wo, Cc, win=None):
    y0, x0, Hc, Wc = win or (0, 0, Hi, Wi)
    _case("resize_aa", id, ("up" if Ho >= Hc else "down", win is not None, Cc > 4), B=B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=Cc, y0=y0, x0=x0, Hc=Hc, Wc=Wc)


OPS["resize_aa"] = Op(_aa_make, _aa_eval, _aa_bounds, _aa_run, dense=True)
_aa_case("up_C4", 2, 14, 19, 58, 77, 4)                                       # the plans: 112 x 152 -> 462 x 616 (and three more scales), C 4
_aa_case("down_C4", 2, 58, 77, 30, 40, 4)                                     # 462 x 616 -> 240 x 320, C 4
_aa_case("down_C192", 1, 29, 39, 7, 10, 192)                                  # 115 x 154 -> 28 x 38, C 192 / 57 x 77, C 384
_aa_case("up_C1536", 1, 7, 10, 14, 19, 1536)                                  # 14 x 19 -> 28 x 38, C 1536
_aa_case("crop_down_C4", 2, 40, 52, 17, 21, 4, win=(3, 5, 33, 41))
_aa_case("crop_up_C4", 1, 20, 27, 31, 41, 4, win=(2, 3, 15, 20))
_aa_case("second_trip", 1, 100, 100, 1460, 1460, 4)                           # more than 256 * 32 * 256 (pixel, 4 channels) items


# ---- ud_nhwc_to_nchw_f32 ----
def _t_make(c):
    return dict(x=_rnd((c["B"], c["hw"], c["C"]), 1))


def _t_eval(c, x, dt):
    return dict(out=x["x"].to(dt).transpose(1, 2).contiguous())


def _t_bounds(c, x, ref):
    return dict(out=torch.zeros(()))


def _t_run(ops, c, x, strided):
    B, hw, Cc = c["B"], c["hw"], c["C"]
    rpi, ld = (hw + 4, Cc + 8) if strided else (hw, Cc)
    xin = torch.full((B, rpi, Cc), float("nan"))
    xin[:, :hw] = x["x"]
    X = lg.poisoned(_dev(xin).reshape(B * rpi, Cc), ld=ld, offset_cols=4 if strided else 0, post_rows=2)
    go = _flat_out(B * Cc * hw, F32, strided)
    ops.check(ops.lib.ud_nhwc_to_nchw_f32(X.data_ptr(), go.ptr(), B, hw, Cc, ld, rpi, ops.cur_stream()))
    return dict(out=go.view.view(B, Cc, hw)), [go]


OPS["nhwc_to_nchw"] = Op(_t_make, _t_eval, _t_bounds, _t_run, dense=True)
_case("nhwc_to_nchw", "C256", (), B=2, hw=77, C=256)                          # the plans: (1, 1452, 256 / 512, ld = C, rows 1456)
_case("nhwc_to_nchw", "odd", (), B=3, hw=37, C=70)                            # neither a multiple of the 64 x 64 tile


# ---- ud_finalize_outputs ----
def _fin_make(c):
    B, nb, Hn, Wn = c["B"], c["nb"], c["Hn"], c["Wn"]
    # every map keeps one sign per channel with neighbours within ~50 % of each other (as the product's maps do): between neighbours of opposite
    # sign |v1 - v0| is the whole sum of the |tap values|, and there the two fp32 roundings of a source coordinate (2^-23 x coordinate) leave the
    # coordinate term (2^-22) a factor 2 of the 4 that the headroom rule asks for -- the other factor 2 comes from |v1 - v0| <= sum / 2
    rays = F.normalize(_rnd((nb, 3, Hn, Wn), 3, 0.15) + torch.tensor([0.6, -0.6, 2.0]).view(1, 3, 1, 1), dim=1)
    return dict(radius=_rnd((B, Hn, Wn), 1, 0.25) + 1.5, conf=_rnd((B, Hn, Wn), 2, 0.25) + 1.0, rays=rays)


def _fin_resample(c, t, dt):
    """F.interpolate to (Hp, Wp) + the crop, as unidepthv2.py:80-89 _postprocess."""
    v = F.interpolate(t.to(dt), size=(c["Hp"], c["Wp"]), mode="bicubic" if c["mode"] == 1 else "bilinear", align_corners=False)
    return v[..., c["pad_t"]:c["pad_t"] + c["Ho"], c["pad_l"]:c["pad_l"] + c["Wo"]]


def _fin_eval(c, x, dt):
    B = c["B"]
    rays = x["rays"].expand(B, -1, -1, -1) if c["nb"] == 1 else x["rays"]
    pts = _fin_resample(c, rays.to(dt) * x["radius"].to(dt).unsqueeze(1), dt)
    rr = _fin_resample(c, x["rays"], dt)
    return dict(confidence=_fin_resample(c, x["conf"].unsqueeze(1), dt)[:, 0], points=pts, depth=pts[:, 2], radius=torch.norm(pts, dim=1),
                rays=rr / torch.norm(rr, dim=1, keepdim=True).clamp(min=1e-5))


def _fin_bounds(c, x, ref):
    B = c["B"]
    rays = x["rays"].expand(B, -1, -1, -1) if c["nb"] == 1 else x["rays"]
    kind = "cubic" if c["mode"] == 1 else "linear"
    wy, wx = _axis_weights(kind, c["Hp"], c["Hn"]), _axis_weights(kind, c["Wp"], c["Wn"])
    wy = tuple(m[c["pad_t"]:c["pad_t"] + c["Ho"]] for m in wy)                  # the crop keeps these output rows / columns
    wx = tuple(m[c["pad_l"]:c["pad_l"] + c["Wo"]] for m in wx)

    def e(t):
        return _separable_bound(t, wy, wx)
    ep = e(rays * x["radius"].unsqueeze(1)) + lg.term_store_f32(ref["points"])  # the product rays x radius is rounded before the resize
    er = e(x["rays"])
    nr = torch.norm(_fin_resample(c, x["rays"], F64), dim=1, keepdim=True).clamp(min=1e-5)
    ep3 = ep.amax(1)
    return dict(confidence=e(x["conf"]), points=ep, depth=ep3, radius=2 * ep3 + lg.term_store_f32(ref["radius"]),
                rays=(2 * er.amax(1, keepdim=True) / nr + 4 * U24).expand_as(ref["rays"]))


def _fin_run(ops, c, x, strided):
    B, nb, Ho, Wo = c["B"], c["nb"], c["Ho"], c["Wo"]
    n = Ho * Wo
    gs = dict(confidence=_flat_out(B * n, F32), radius=_flat_out(B * n, F32), depth=_flat_out(B * n, F32), points=_flat_out(B * 3 * n, F32),
              rays=_flat_out(nb * 3 * n, F32))
    d = ops.mk(ops.UdFinalize, radius_net=_flat_in(_dev(x["radius"])), conf_net=_flat_in(_dev(x["conf"])), rays_net=_flat_in(_dev(x["rays"])),
               **{k: g.view for k, g in gs.items()}, B=B, nb_rays=nb, Hn=c["Hn"], Wn=c["Wn"], Hp=c["Hp"], Wp=c["Wp"], pad_l=c["pad_l"], pad_t=c["pad_t"],
               Ho=Ho, Wo=Wo, mode=c["mode"])
    ops.check(ops.lib.ud_finalize_outputs(C.byref(d), ops.cur_stream()))
    shp = dict(confidence=(B, Ho, Wo), radius=(B, Ho, Wo), depth=(B, Ho, Wo), points=(B, 3, Ho, Wo), rays=(nb, 3, Ho, Wo))
    return {k: g.view.view(shp[k]) for k, g in gs.items()}, list(gs.values())


OPS["finalize"] = Op(_fin_make, _fin_eval, _fin_bounds, _fin_run)
for _mode in (0, 1):
    _nm = "bicubic" if _mode else "bilinear"
    _case("finalize", f"{_nm}_padded_nb1", (_mode,), B=2, nb=1, Hn=28, Wn=42, Hp=37, Wp=50, pad_l=0, pad_t=0, Ho=37, Wo=50, mode=_mode)
    _case("finalize", f"{_nm}_cropped_nbB", (_mode,), B=2, nb=2, Hn=28, Wn=42, Hp=45, Wp=61, pad_l=5, pad_t=3, Ho=39, Wo=50, mode=_mode)
    _case("finalize", f"{_nm}_down", (_mode,), B=1, nb=1, Hn=42, Wn=56, Hp=24, Wp=32, pad_l=2, pad_t=1, Ho=20, Wo=29, mode=_mode)
_case("finalize", "second_trip", (0,), B=2, nb=2, Hn=42, Wn=56, Hp=1030, Wp=1030, pad_l=0, pad_t=0, Ho=1030, Wo=1030, mode=0)    # more than 256 * 32 blocks


# ---- V1 PREPROCESS: [/255], ImageNet normalisation, antialiased resize to (h, w), zero pad to (Hn, Wn) ----
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _pre_make(c):
    g = torch.Generator().manual_seed(1)
    if c["is_u8"] and "second_trip" in c["id"]:                               # a smooth image: see _ac_make on the maps of ~10^6 elements
        return dict(rgb=torch.randint(96, 160, (c["B"], 3, c["H"], c["W"]), dtype=torch.uint8, generator=g))
    if c["is_u8"]:
        return dict(rgb=torch.randint(0, 256, (c["B"], 3, c["H"], c["W"]), dtype=torch.uint8, generator=g))
    return dict(rgb=torch.rand(c["B"], 3, c["H"], c["W"], generator=g) * (255.0 if c["div255"] else 1.0))


def _pre_pixels(c, x, dt, absval=False):
    """The source pixels the resize sees; absval: every term on absolute values."""
    v = x["rgb"].to(dt)
    if c["div255"]:
        v = v / 255
    if c["normalize"]:
        m, s = torch.tensor(_MEAN, dtype=F32).to(dt).view(1, 3, 1, 1), torch.tensor(_STD, dtype=dt).view(1, 3, 1, 1)
        v = (v + m) / s if absval else (v - m) / s
    return v


def _pre_eval(c, x, dt):
    v = F.interpolate(_pre_pixels(c, x, dt), size=(c["h"], c["w"]), mode="bilinear", align_corners=False, antialias=True)
    pl, pt = c["pad_l"], c["pad_t"]
    return dict(out=F.pad(v, (pl, c["Wn"] - c["w"] - pl, pt, c["Hn"] - c["h"] - pt)))


def _pre_bounds(c, x, ref):
    wy, wx = _axis_weights("aa", c["h"], c["H"]), _axis_weights("aa", c["w"], c["W"])
    px = _pre_pixels(c, x, F64, absval=True)
    # the kernel multiplies by fp32(1 / std) and fp32(1 / 255) where the statement divides: 2^-23 relative on top of the sums
    e = _separable_bound(px, wy, wx) + 4 * U24 * _separable(px, wy[0], wx[0])
    pl, pt = c["pad_l"], c["pad_t"]
    return dict(out=F.pad(e, (pl, c["Wn"] - c["w"] - pl, pt, c["Hn"] - c["h"] - pt)))       # the zero padding is exact


def _pre_run(ops, c, x, strided):
    B, Hn, Wn = c["B"], c["Hn"], c["Wn"]
    rgb = _dev(x["rgb"]) if c["is_u8"] else _flat_in(_dev(x["rgb"]))
    go = _flat_out(B * 3 * Hn * Wn, F32)
    _v1(ops, K_PREPROCESS, a=rgb, out=go.view, i=(B, c["H"], c["W"], c["h"], c["w"], Hn, Wn, c["pad_l"], c["pad_t"], c["is_u8"], c["div255"], c["normalize"]))
    return dict(out=go.view.view(B, 3, Hn, Wn)), [go]


OPS["preprocess_v1"] = Op(_pre_make, _pre_eval, _pre_bounds, _pre_run)
# the plan: (1, 240, 320, 462, 616, 462, 616, 0, 0, is_u8 1, div255 0, normalize 1) -- u8 up-sampling; the flags act independently in the kernel
_case("preprocess_v1", "u8_plan", (1, 0, 1), B=1, H=24, W=32, h=46, w=61, Hn=46, Wn=61, pad_l=0, pad_t=0, is_u8=1, div255=0, normalize=1)
_case("preprocess_v1", "float_up", (0, 0, 1), B=2, H=24, W=32, h=46, w=61, Hn=46, Wn=61, pad_l=0, pad_t=0, is_u8=0, div255=0, normalize=1)
_case("preprocess_v1", "u8_padded_down", (1, 1, 1), B=2, H=61, W=83, h=28, w=38, Hn=35, Wn=42, pad_l=3, pad_t=2, is_u8=1, div255=1, normalize=1)
_case("preprocess_v1", "float255_padded", (0, 1, 1), B=1, H=30, W=41, h=33, w=45, Hn=42, Wn=56, pad_l=6, pad_t=4, is_u8=0, div255=1, normalize=1)
_case("preprocess_v1", "second_trip", (1, 1, 0), B=2, H=30, W=40, h=600, w=610, Hn=602, Wn=616, pad_l=3, pad_t=1, is_u8=1, div255=1, normalize=0)


# ======================================================================================================================================
# C. LayerNorm-statistic and embedding outputs
# ======================================================================================================================================
# ---- ud_layernorm_patchify2 ----
def _lp_make(c):
    x = _rnd((c["B"], c["H"], c["W"], c["C"]), 1) * 1.5 + 0.4
    return dict(x=_lowvar(x, c["eps"], (slice(None), slice(c["H"] // 2, c["H"]))))


def _lp_arrange(c, y):
    B, H, W, Cc = y.shape
    Ho, Wo = H // 2, W // 2
    y = y[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, Cc).permute(0, 1, 3, 2, 4, 5)
    return y.reshape(B * Ho * Wo, 4 * Cc)


def _lp_eval(c, x, dt, eps_scale=1.0):
    return dict(out=_lp_arrange(c, F.layer_norm(x["x"].to(dt), (c["C"],), eps=c["eps"] * eps_scale)))


def _lp_bounds(c, x, ref):
    return dict(out=_lp_arrange(c, _ln_bound(x["x"].double(), 0.0, c["eps"])))


def _lp_run(ops, c, x, strided):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    ldo = 4 * Cc + (264 if strided else 0)
    go = lg.guarded(B * (H // 2) * (W // 2), 4 * Cc, ldo, F16, offset_cols=8 if strided else 0)
    ops.check(ops.lib.ud_layernorm_patchify2(_flat_in(_dev(x["x"])).data_ptr(), go.ptr(), B, H, W, Cc, ldo, c["eps"], ops.cur_stream()))
    return dict(out=go.view), [go]


OPS["ln_patchify2"] = Op(_lp_make, _lp_eval, _lp_bounds, _lp_run, dense=True, stores=lambda c: dict(out="f16"))
for _cc, _nit in ((192, 1), (384, 2), (768, 4), (1536, 8)):                   # the plans: C 192 / 384 / 768; one case per template width
    _case("ln_patchify2", f"C{_cc}", (_nit,), B=2, H=7, W=9, C=_cc, eps=1e-6)


# ---- ud_patchify4_nchw ----
def _p4_make(c):
    return dict(img=_rnd((c["B"], 3, c["H"], c["W"]), 1))


def _p4_eval(c, x, dt):
    B, H, W = c["B"], c["H"], c["W"]
    v = x["img"].to(dt)[:, :, :H // 4 * 4, :W // 4 * 4]
    return dict(out=F.unfold(v, 4, stride=4).transpose(1, 2).reshape(-1, 48))


def _p4_bounds(c, x, ref):
    return dict(out=torch.zeros(()))                                          # a conversion: nothing but the store


def _p4_run(ops, c, x, strided):
    B, H, W = c["B"], c["H"], c["W"]
    ldo = 64 + (72 if strided else 0)                                         # the product's ldo is 64: columns 48..63 must keep what they hold
    go = lg.guarded(B * (H // 4) * (W // 4), 48, ldo, F16, offset_cols=8 if strided else 0)
    ops.check(ops.lib.ud_patchify4_nchw(_flat_in(_dev(x["img"])).data_ptr(), go.ptr(), B, H, W, ldo, ops.cur_stream()))
    return dict(out=go.view), [go]


OPS["patchify4"] = Op(_p4_make, _p4_eval, _p4_bounds, _p4_run, dense=True, stores=lambda c: dict(out="f16"))
_case("patchify4", "ld64", (), B=2, H=22, W=31)                               # the plan: (1, 462, 616, 64)
_case("patchify4", "second_trip", (), B=1, H=600, W=604)                      # more than 256 * 16 blocks


# ---- ud_dwconv7_nhwc_f32 ----
def _dw_make(c):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    x = _rnd((B, H, W, Cc), 1)
    if c.get("final"):
        _lowvar(x, c["eps"] * 49, (slice(None), slice(H // 2, H)))            # 49 taps of ~unit weight: the OUTPUT's deviation is ~10 sqrt(eps) there
    return dict(x=x, w=_rnd((49, Cc), 2, 1.0 / 7), bias=_rnd((Cc,), 3, 0.01 if c.get("final") else 1.0))


def _dw_conv(c, x, dt, absval=False):
    Cc = c["C"]
    f = (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))
    w = f(x["w"]).t().reshape(Cc, 1, 7, 7)
    return F.conv2d(f(x["x"]).permute(0, 3, 1, 2), w, f(x["bias"]), padding=3, groups=Cc).permute(0, 2, 3, 1)


def _dw_eval(c, x, dt, eps_scale=1.0):
    y = _dw_conv(c, x, dt)
    out = {}
    if c["y"]:
        out["y"] = y
    if c.get("y16"):
        out["y16"] = y
        B, H, W, Cc = y.shape
        s = y.reshape(B * H * W, Cc // 64, 64)
        out["stats"] = torch.stack([s.sum(-1), (s * s).sum(-1)], -1)
        if c.get("final"):
            m = y.mean(-1)
            rstd = torch.rsqrt((y * y).mean(-1) - m * m + c["eps"] * eps_scale) if dt == F32 else torch.rsqrt(y.var(-1, unbiased=False) + c["eps"] * eps_scale)
            out["final"] = torch.stack([rstd, -m * rstd], -1).reshape(B * H * W, 2)
    return out


def _dw_bounds(c, x, ref):
    e = lg.term_rounding(_dw_conv(c, x, F64, absval=True), 49)
    b = {}
    if c["y"]:
        b["y"] = e
    if c.get("y16"):
        y = _dw_conv(c, x, F64)
        B, H, W, Cc = y.shape
        b["y16"] = e
        ys, es = y.reshape(B * H * W, Cc // 64, 64), e.reshape(B * H * W, Cc // 64, 64)
        d1 = es.sum(-1) + lg.term_rounding(ys.abs().sum(-1), 64)
        d2 = (2 * ys.abs() * es).sum(-1) + lg.term_rounding((ys * ys).sum(-1), 64)
        b["stats"] = torch.stack([d1, d2], -1)
        if c.get("final"):
            # (rstd, -mean rstd) from the sums S1, S2 over C: var = S2 / C - mean^2 in fp32 cancels against mean^2, so
            # d var <= (d S2 + rounding) / C + 2 |mean| d mean + 2^-23 (S2 / C + mean^2);  d rstd = rstd^3 d var / 2
            yy = y.reshape(B * H * W, Cc)
            m, msq = yy.mean(-1), (yy * yy).mean(-1)
            rstd = torch.rsqrt(yy.var(-1, unbiased=False) + c["eps"])
            dm = d1.sum(-1) / Cc + lg.term_rounding(yy.abs().mean(-1), Cc // 64)
            dv = d2.sum(-1) / Cc + lg.term_rounding(msq, Cc // 64) + 2 * m.abs() * dm + 4 * U24 * (msq + m * m)
            dr = 0.5 * rstd ** 3 * dv + 4 * U24 * rstd
            b["final"] = torch.stack([dr, m.abs() * dr + rstd * dm + 4 * U24 * (m * rstd).abs()], -1)
    return b


def _dw_run(ops, c, x, strided):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    P = B * H * W
    ldx, ldy, ldy16 = (Cc + 12, Cc + 20, Cc + 24) if strided else (Cc, Cc, Cc)
    X = lg.poisoned(_dev(x["x"]).reshape(P, Cc), ld=ldx, offset_cols=4 if strided else 0, post_rows=2)
    kw = dict(x=X, w=_flat_in(_dev(x["w"])), bias=_flat_in(_dev(x["bias"])), B=B, H=H, W=W, C=Cc, ldx=ldx, ldy=ldy)
    gs, out = [], {}
    if c["y"]:
        gy = lg.guarded(P, Cc, ldy, F32, offset_cols=4 if strided else 0)
        kw["y"], out["y"] = gy.view, gy.view.view(B, H, W, Cc)
        gs.append(gy)
    if c.get("y16"):
        g16 = lg.guarded(P, Cc, ldy16, F16, offset_cols=8 if strided else 0)
        gst = lg.guarded(P, 2 * (Cc // 64), 2 * (Cc // 64), F32)
        kw.update(y16=g16.view, ldy16=ldy16, stats_out=gst.view)
        out["y16"], out["stats"] = g16.view.view(B, H, W, Cc), gst.view.view(P, Cc // 64, 2)
        gs += [g16, gst]
        if c.get("final"):
            gf = lg.guarded(P, 2, 2, F32)
            tick = torch.zeros(B * ((H + 7) // 8) * ((W + 15) // 16) + 64, dtype=torch.int32, device="cuda")
            kw.update(stats_final=gf.view, stats_ticket=tick, ln_eps=c["eps"])
            out["final"] = gf.view
            gs.append(gf)
    d = ops.mk(ops.UdDwConv7, **kw)
    ops.check(ops.lib.ud_dwconv7_nhwc_f32(C.byref(d), ops.cur_stream()))
    if c.get("final"):
        torch.cuda.synchronize()
        assert int(tick.abs().sum()) == 0, f"{c['id']}: the tickets did not return to zero"
    return out, gs


def _dw_class(Cc, y, y16, final):
    return ("lds" if Cc % 64 == 0 else "plain", bool(y), bool(y16), bool(final), Cc)


OPS["dwconv7"] = Op(_dw_make, _dw_eval, _dw_bounds, _dw_run, dense=True, stores=lambda c: dict(y16="f16") if c.get("y16") else {})
for _id, _kw in (("lds_C128", dict(B=2, H=11, W=19, C=128)), ("lds_C768", dict(B=1, H=9, W=17, C=768)), ("lds_C1536", dict(B=1, H=7, W=5, C=1536)),
                 ("lds_C256", dict(B=1, H=9, W=17, C=256)), ("lds_C384", dict(B=1, H=8, W=18, C=384)), ("lds_C512", dict(B=1, H=10, W=9, C=512)),
                 ("plain_C96", dict(B=2, H=11, W=19, C=96)), ("plain_C36", dict(B=1, H=5, W=9, C=36))):
    _case("dwconv7", _id, _dw_class(_kw["C"], 1, 0, 0), y=1, **_kw)             # the plans: y only at C 128, 256, 384, 512, 768, 1536 (LDS kernel)
_case("dwconv7", "y16_stats", _dw_class(192, 0, 1, 0), B=2, H=11, W=19, C=192, y=0, y16=1, eps=1e-6)
_case("dwconv7", "y16_stats_final", _dw_class(192, 0, 1, 1), B=2, H=13, W=21, C=192, y=0, y16=1, final=1, eps=1e-6)     # the plan: (115 x 154, C 192, tickets)
_case("dwconv7", "y_y16_stats_final", _dw_class(256, 1, 1, 1), B=1, H=9, W=17, C=256, y=1, y16=1, final=1, eps=1e-6)
# the batched V1 ConvNeXt-L plans (batch 2 at 200 x 360: C 384; batch 16 at 480 x 640: C 384 and 768): 6 / 12 channel blocks draw a pixel tile's tickets
_case("dwconv7", "y16_stats_final_C384", _dw_class(384, 0, 1, 1), B=2, H=9, W=17, C=384, y=0, y16=1, final=1, eps=1e-6)
_case("dwconv7", "y16_stats_final_C768", _dw_class(768, 0, 1, 1), B=1, H=9, W=17, C=768, y=0, y16=1, final=1, eps=1e-6)


# ======================================================================================================================================
# D. small attention and softmax
# ======================================================================================================================================
# ---- V1 SOFTMAX ----
# T_SOFTMAX: unit 2^-24 p (relative); torch fp32 softmax against fp64 on these cases: 20.01 (the argument (s - max) scale reaches ~ -20,
# and d exp = exp d arg)
T_SOFTMAX = 81.0


def _sm_kernel(N, ldi, ldo, f32):
    if not f32 and N % 4 == 0 and ldi % 4 == 0 and ldo % 4 == 0 and 256 < N <= 5120:
        return "reg5" if N <= 1280 else "reg20"
    return "generic"


def _sm_make(c):
    return dict(s=_rnd((c["rows"], c["N"]), 1, 2.0))


def _sm_eval(c, x, dt, pad_garbage=False):
    p = torch.softmax(x["s"].to(dt) * torch.tensor(c["scale"], dtype=F32).to(dt), -1)
    pad = torch.zeros(c["rows"], c["ldo"] - c["N"], dtype=p.dtype)
    if pad_garbage:
        pad = pad + 2.0 ** -14                                                  # a stale small probability left in the K padding
    return dict(p=p, pad=pad)


def _sm_bounds(c, x, ref):
    return dict(p=T_SOFTMAX * U24 * ref["p"], pad=torch.zeros(()))


def _sm_run(ops, c, x, strided):
    rows, N, ldo, f32 = c["rows"], c["N"], c["ldo"], c["f32"]
    ldi = N + (c.get("ipad", 8) if strided else 0)
    S = lg.poisoned(_dev(x["s"]), ld=ldi, post_rows=3)
    go = lg.guarded(rows, ldo, ldo, F32 if f32 else F16)                      # ldo is the row stride AND the zero-filled width
    assert (_sm_kernel(N, ldi, ldo, f32), N > 5120) == (c["cls"][1], c["cls"][3]), (c["id"], _sm_kernel(N, ldi, ldo, f32))
    _v1(ops, K_SOFTMAX, a=S, out=go.view, i=(rows & 0x7fffffff, N, ldi, ldo, f32, rows >> 31), f=(c["scale"],))
    return dict(p=go.view[:, :N], pad=go.view[:, N:]), [go]


OPS["softmax"] = Op(_sm_make, _sm_eval, _sm_bounds, _sm_run, stores=lambda c: {} if c["f32"] else dict(p="f16"))
_case("softmax", "generic_N200", ("generic", 0, False), rows=9, N=200, ldo=208, f32=0, scale=1.0)
_case("softmax", "generic_odd", ("generic", 0, False), rows=7, N=1063, ldo=1088, f32=0, scale=0.7, ipad=5)
_case("softmax", "reg5_N1064", ("reg5", 0, False), rows=11, N=1064, ldo=1088, f32=0, scale=1.0)         # the plans: (1064, 1064, 1064, 1088), (1452, 1452, 1452, 1472)
_case("softmax", "reg5_N1280", ("reg5", 0, False), rows=6, N=1280, ldo=1280, f32=0, scale=1.3)
_case("softmax", "reg20_N1452", ("reg20", 0, False), rows=5, N=1452, ldo=1472, f32=0, scale=1.0)
_case("softmax", "reg20_N4256", ("reg20", 0, False), rows=6, N=4256, ldo=4288, f32=0, scale=1.0)         # the plan: (1064, 4256, 4256, 4288)
_case("softmax", "reg20_N5120", ("reg20", 0, False), rows=5, N=5120, ldo=5120, f32=0, scale=1.0)         # the last register of the row
_case("softmax", "reg20_N5120_pad", ("reg20", 0, False), rows=5, N=5120, ldo=5184, f32=0, scale=1.0)     # zero fill past the registers' span
_case("softmax", "generic_N5808", ("generic", 0, True), rows=3, N=5808, ldo=5824, f32=0, scale=1.0)      # the plan: (1452, 5808, 5808, 5824), past the registers
_case("softmax", "f32_N300", ("generic", 1, False), rows=9, N=300, ldo=320, f32=1, scale=1.0)
_case("softmax", "f32_N1064", ("generic", 1, False), rows=5, N=1064, ldo=1088, f32=1, scale=0.5)


# ---- small attentions: shared statement ----
# T_ATT: unit 2^-24 p (relative) per probability; torch fp32 softmax of these cases' scores against fp64: 7.88
T_ATT = 32.0


def _att(q, k, v, scale, dt):
    """softmax(q k^T scale) v over the last two axes at `dt`; also returns what the bound needs."""
    s = (q.to(dt) @ k.to(dt).transpose(-1, -2)) * torch.tensor(scale, dtype=F32).to(dt)
    p = torch.softmax(s, -1)
    return p @ v.to(dt), s, p


def _att_bound(q, k, v, scale):
    o, s, p = _att(q, k, v, scale, F64)
    D = q.shape[-1]
    ds = lg.term_rounding((q.double().abs() @ k.double().abs().transpose(-1, -2)) * scale, D)         # a score's own rounding
    rel = 2 * (ds + ds.amax(-1, keepdim=True)) + T_ATT * U24                                              # d p / p
    mag = p @ v.double().abs()
    return (p * rel) @ v.double().abs() + lg.term_rounding(mag, k.shape[-2]) + lg.term_store_f32(o)


# ---- V1 HEAD_MIX: per token, the h head vectors attend to each other ----
def _hm_make(c):
    M, h = c["M"], c["h"]
    return dict(q=_rnd((M, h, 64), 1), k=_rnd((M, h, 64), 2), v=_rnd((M, h, 64), 3))


def _hm_eval(c, x, dt):
    return dict(out=_att(x["q"], x["k"], x["v"], c["scale"], dt)[0].reshape(c["M"], -1))


def _hm_bounds(c, x, ref):
    return dict(out=_att_bound(x["q"], x["k"], x["v"], c["scale"]).reshape(c["M"], -1))


def _hm_run(ops, c, x, strided):
    M, h = c["M"], c["h"]
    w = h * 64
    ldq, ldkv, ldo = (w + 68, 2 * w + 36, w + 136) if strided else (w, 2 * w, w)
    Q = lg.poisoned(_dev(x["q"]).reshape(M, w), ld=ldq, offset_cols=4 if strided else 0, post_rows=2)
    KV = lg.poisoned(torch.cat([_dev(x["k"]).reshape(M, w), _dev(x["v"]).reshape(M, w)], 1), ld=ldkv, offset_cols=4 if strided else 0, post_rows=2)
    go = lg.guarded(M, w, ldo, F16, offset_cols=8 if strided else 0)
    _v1(ops, K_HEAD_MIX, a=Q, b=KV, out=go.view, i=(M, h, ldq, ldkv, ldo), f=(c["scale"],))
    return dict(out=go.view), [go]


OPS["head_mix"] = Op(_hm_make, _hm_eval, _hm_bounds, _hm_run, dense=True, stores=lambda c: dict(out="f16"))
for _h in (2, 4, 8):                     # the plans: h 2 (ld 128 / 256 / 128) and h 4 (256 / 512 / 256); the width is 64 h, so h is the bucket of C
    _case("head_mix", f"h{_h}", (_h,), M=301, h=_h, scale=0.125)
_case("head_mix", "second_trip", (2,), M=4 * 8192 + 37, h=2, scale=0.125)      # the grid is capped at 8192 blocks of 4 tokens


# ---- V1 ATTN_FEWQ: T <= 8 queries against Nk keys, one head of width D; kv fp16 [K | V] ----
def _fq_make(c):
    B, T, Nk, D = c["B"], c["T"], c["Nk"], c["D"]
    return dict(q=_rnd((B, T, D), 1), k=_rnd((B, Nk, D), 2).half(), v=_rnd((B, Nk, D), 3).half())


def _fq_eval(c, x, dt):
    return dict(out=_att(x["q"], x["k"], x["v"], c["scale"], dt)[0])


def _fq_bounds(c, x, ref):
    return dict(out=_att_bound(x["q"], x["k"], x["v"], c["scale"]))


def _fq_run(ops, c, x, strided):
    B, T, Nk, D = c["B"], c["T"], c["Nk"], c["D"]
    q = _flat_in(_dev(x["q"]))
    kv = _flat_in(torch.cat([_dev(x["k"]), _dev(x["v"])], -1))
    go = lg.guarded(B * T, D, D, F32)
    scratch = None
    if c["chunked"]:
        scratch = torch.full((B * -(-Nk // 64) * T * (D + 2) + 64,), float("nan"), device="cuda")
    _v1(ops, K_ATTN_FEWQ, a=q, b=kv, c=scratch, out=go.view, i=(B, T, Nk, D), f=(c["scale"],))
    return dict(out=go.view.view(B, T, D)), [go]


OPS["attn_fewq"] = Op(_fq_make, _fq_eval, _fq_bounds, _fq_run)
for _ch in (0, 1):                                                            # the plan: chunked, (1, 4, 4260, 512), scale 512^-0.5
    _case("attn_fewq", f"T4_chunked{_ch}", (_ch,), B=2, T=4, Nk=533, D=512, scale=512 ** -0.5, chunked=_ch)
    _case("attn_fewq", f"T8_chunked{_ch}", (_ch,), B=1, T=8, Nk=64, D=64, scale=0.125, chunked=_ch)
_case("attn_fewq", "T1_Nk1", (1,), B=3, T=1, Nk=1, D=8, scale=1.0, chunked=1)


# ---- ud_attention_small_f32: T <= 8 tokens, H heads; q [B T, C], kv [B T, 2 C] ----
def _as_make(c):
    B, T, H, Cc = c["B"], c["T"], c["H"], c["C"]
    return dict(q=_rnd((B, T, Cc), 1), k=_rnd((B, T, Cc), 2), v=_rnd((B, T, Cc), 3))


def _as_heads(c, t):
    B, T, H, Cc = c["B"], c["T"], c["H"], c["C"]
    return t.view(B, T, H, Cc // H).transpose(1, 2)


def _as_eval(c, x, dt):
    o = _att(_as_heads(c, x["q"]), _as_heads(c, x["k"]), _as_heads(c, x["v"]), c["scale"], dt)[0]
    return dict(out=o.transpose(1, 2).reshape(c["B"], c["T"], c["C"]))


def _as_bounds(c, x, ref):
    b = _att_bound(_as_heads(c, x["q"]), _as_heads(c, x["k"]), _as_heads(c, x["v"]), c["scale"])
    return dict(out=b.transpose(1, 2).reshape(c["B"], c["T"], c["C"]))


def _as_run(ops, c, x, strided):
    B, T, H, Cc = c["B"], c["T"], c["H"], c["C"]
    q = _flat_in(_dev(x["q"]))
    kv = _flat_in(torch.cat([_dev(x["k"]), _dev(x["v"])], -1))
    go = lg.guarded(B * T, Cc, Cc, F32)
    ops.check(ops.lib.ud_attention_small_f32(q.data_ptr(), kv.data_ptr(), go.ptr(), B, T, H, Cc, c["scale"], ops.cur_stream()))
    return dict(out=go.view.view(B, T, Cc)), [go]


OPS["attention_small"] = Op(_as_make, _as_eval, _as_bounds, _as_run)
_case("attention_small", "T4_H8_C512", (), B=3, T=4, H=8, C=512, scale=0.125)          # the plan: (1, 4, 8, 512, 0.125)
_case("attention_small", "T8_H4_C96", (), B=2, T=8, H=4, C=96, scale=24 ** -0.5)        # head width 24 < 64 lanes
_case("attention_small", "T1", (), B=2, T=1, H=2, C=128, scale=0.125)


# ---- V1 OUT_CONV3: exp(clamp(conv3x3 to one channel + bias, -10, 10)), out [pixels, ldo] column 0 ----
# T_EXP: unit 2^-24 out (relative); torch fp32 exp of these cases' clamped pre-activations against fp64: 0.99
T_EXP = 4.0


def _oc_make(c):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    return dict(x=_rnd((B, H, W, Cc), 1), w=_rnd((9, Cc), 2, c.get("wscale", 1.0) / math.sqrt(9 * Cc)))


def _oc_pre(c, x, dt, absval=False):
    f = (lambda t: t.to(dt).abs()) if absval else (lambda t: t.to(dt))
    w = f(x["w"]).view(3, 3, c["C"]).permute(2, 0, 1).unsqueeze(0)
    return F.conv2d(f(x["x"]).permute(0, 3, 1, 2), w, padding=1)[:, 0] + (abs(c["bias"]) if absval else torch.tensor(c["bias"], dtype=F32).to(dt))


def _oc_eval(c, x, dt):
    return dict(out=torch.exp(_oc_pre(c, x, dt).clamp(-10, 10)).reshape(-1, 1))


def _oc_bounds(c, x, ref):
    d = lg.term_rounding(_oc_pre(c, x, F64, absval=True), 9 * c["C"]).reshape(-1, 1)
    return dict(out=ref["out"] * (torch.expm1(d) + T_EXP * U24))             # d exp(y) = exp(y) (e^dy - 1), plus expf itself


def _oc_run(ops, c, x, strided):
    B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
    go = lg.guarded(B * H * W, 1, 4, F32)                                    # the product's ldo: columns 1..3 are guard elements
    _v1(ops, K_OUT_CONV3, a=_flat_in(_dev(x["x"])), b=_flat_in(_dev(x["w"])), out=go.view, i=(B, H, W, Cc, 4), f=(c["bias"],))
    return dict(out=go.view), [go]


OPS["out_conv3"] = Op(_oc_make, _oc_eval, _oc_bounds, _oc_run)
_case("out_conv3", "C64", (64,), B=2, H=19, W=45, C=64, bias=-0.12)              # the plans: C 64 / 128 / 256, ldo 4
_case("out_conv3", "C128", (128,), B=1, H=10, W=35, C=128, bias=-0.05)
_case("out_conv3", "C256", (256,), B=1, H=9, W=33, C=256, bias=0.03)
_case("out_conv3", "C36_clamped", (36,), B=1, H=8, W=32, C=36, bias=0.5, wscale=8.0)        # pre-activations reach both clamps; C not a multiple of 32


# ---- V1 POINTS: z map + K33 -> points, depth ----
# T_PTS: unit 2^-24 (|x| + |y| + |z|) per point; torch fp32 of the atan2 / acos / tan chain against fp64 on these cases: 2.89
T_PTS = 12.0


def _pt_make(c):
    B, H, W, nK = c["B"], c["H"], c["W"], c["nK"]
    K = torch.zeros(nK, 9)
    for b in range(nK):
        K[b, 0], K[b, 4], K[b, 2], K[b, 5], K[b, 8] = 0.8 * W + 3 * b, 0.9 * W, 0.5 * W + b, 0.45 * H, 1.0
    return dict(z=_rnd((B * H * W, 1), 1).abs() + 0.5, K=K)


def _pt_eval(c, x, dt):
    B, H, W, nK = c["B"], c["H"], c["W"], c["nK"]
    K = x["K"].to(dt)[[0] * B if nK == 1 else list(range(B))]
    u = (torch.arange(W, dtype=dt) + 0.5).view(1, 1, W)
    v = (torch.arange(H, dtype=dt) + 0.5).view(1, H, 1)
    xx = ((u - K[:, 2].view(B, 1, 1)) / K[:, 0].view(B, 1, 1)).expand(B, H, W)
    yy = ((v - K[:, 5].view(B, 1, 1)) / K[:, 4].view(B, 1, 1)).expand(B, H, W)
    r = F.normalize(torch.stack([xx, yy, torch.ones_like(xx)], 1), dim=1)
    theta, phi = torch.atan2(r[:, 0], r[:, 2]), torch.acos(r[:, 1])
    z = x["z"].to(dt).view(B, H, W)
    return dict(points=torch.stack([z * torch.tan(theta), z / torch.tan(phi) / torch.cos(theta), z], 1), depth=z.unsqueeze(1).clone())


def _pt_bounds(c, x, ref):
    p = ref["points"].abs()
    return dict(points=(T_PTS * U24 * p.sum(1, keepdim=True)).expand_as(p) * torch.tensor([1.0, 1.0, 0.0]).view(1, 3, 1, 1), depth=torch.zeros(()))


def _pt_run(ops, c, x, strided):
    B, H, W, nK = c["B"], c["H"], c["W"], c["nK"]
    Z = lg.poisoned(_dev(x["z"]), ld=4, post_rows=4)                         # the product's ldz: depth is column 0 of 4-wide rows
    gp, gd = _flat_out(B * 3 * H * W, F32), _flat_out(B * H * W, F32)
    _v1(ops, K_POINTS, a=Z, b=lg.poisoned(_dev(x["K"]), post_rows=1), out=gp.view, out2=gd.view, i=(B, H, W, 4, nK))
    return dict(points=gp.view.view(B, 3, H, W), depth=gd.view.view(B, 1, H, W)), [gp, gd]


OPS["points"] = Op(_pt_make, _pt_eval, _pt_bounds, _pt_run)
_case("points", "nK1", (), B=2, H=30, W=41, nK=1)
_case("points", "nKB", (), B=3, H=17, W=23, nK=3)
_case("points", "second_trip", (), B=1, H=1460, W=1461, nK=1)


# ======================================================================================================================================
# C (continued). ray embeddings
# ======================================================================================================================================
# T_EMB: unit 2^-24, absolute error of one sine band BEFORE the LayerNorm, per unit of band frequency x pi (|d sin(a s pi)| <= s pi |d a| + ...):
# torch fp32 of acos / atan2 of the antialiased, renormalised ray against fp64 on these cases, in 2^-24 (1 + |angle|): 5.42
T_EMB = 22.0


def _re_rays(c):
    nb, Hn, Wn = c["nb"], c["Hn"], c["Wn"]
    u = (torch.arange(Wn) + 0.5 - 0.47 * Wn).view(1, 1, Wn) / (0.8 * Wn)
    v = (torch.arange(Hn) + 0.5 - 0.52 * Hn).view(1, Hn, 1) / (0.8 * Wn)
    sc = (1 + 0.3 * torch.arange(nb)).view(nb, 1, 1)
    return F.normalize(torch.stack([(u * sc).expand(nb, Hn, Wn), (v * sc).expand(nb, Hn, Wn), torch.ones(nb, Hn, Wn)], 1), dim=1)


def _re_make(c):
    nbands = c["C"] // 2
    return dict(rays=_re_rays(c), scales=2.0 ** torch.linspace(0.0, math.log2(max(c["h"], c["w"]) // 2), steps=nbands))


def _re_angles(c, x, dt):
    nb, h, w = c["nb"], c["h"], c["w"]
    t = F.interpolate(x["rays"].to(dt), size=(h, w), mode="bilinear", align_corners=False, antialias=True) if (c["Hn"], c["Wn"]) != (h, w) else x["rays"].to(dt)
    e = t.reshape(nb, 3, h * w).permute(0, 2, 1)
    e = e / torch.norm(e, dim=-1, keepdim=True).clip(min=1e-4)
    xx, yy, zz = e[..., 0], e[..., 1], e[..., 2]
    xc = xx.abs().clip(min=1e-3) * (2 * (xx >= 0).to(dt) - 1)
    return torch.stack([torch.acos(zz), torch.atan2(yy, xc)], -1)            # [nb, hw, 2]


def _re_eval(c, x, dt, eps_scale=1.0):
    ang = _re_angles(c, x, dt)
    v = (ang.unsqueeze(-1) * x["scales"].to(dt) * math.pi).sin().flatten(-2)  # [polar bands | azimuth bands], oracle/restate.py _embed_rays
    return dict(out=_ln(v, c["eps"] * eps_scale))


def _re_bounds(c, x, ref):
    ang = _re_angles(c, x, F64)
    sc = x["scales"].double() * math.pi
    arg = ang.unsqueeze(-1) * sc
    # d sin(a s pi): the angle's error times s pi, the product's two roundings (2^-23 |arg|), and sinf's own few ulp at |arg| up to ~70
    e = (T_EMB * U24 * sc * (1 + ang.abs().unsqueeze(-1)) + 4 * U24 * arg.abs() + 4 * U24).flatten(-2)
    return dict(out=_ln_bound(arg.sin().flatten(-2), e, c["eps"]))


def _re_run(ops, c, x, strided):
    nb, h, w, Cc = c["nb"], c["h"], c["w"], c["C"]
    rpi, ldy = (h * w + 4, Cc + 40) if strided else (h * w, Cc)
    rows = (torch.arange(nb)[:, None] * rpi + torch.arange(h * w)[None]).reshape(-1)
    go = lg.guarded(nb * rpi, Cc, ldy, F16, offset_cols=8 if strided else 0, rows_inside=_dev(rows))
    d = ops.mk(ops.UdRayEmbed, rays=_flat_in(_dev(x["rays"])), scales=_flat_in(_dev(x["scales"])), xhat=go.view, nb=nb, Hn=c["Hn"], Wn=c["Wn"], h=h, w=w, C=Cc,
               ldy=ldy, rows_per_img=rpi, eps=c["eps"])
    ops.check(ops.lib.ud_ray_embed(C.byref(d), ops.cur_stream()))
    return dict(out=go.view[_dev(rows)].view(nb, h * w, Cc)), [go]


OPS["ray_embed"] = Op(_re_make, _re_eval, _re_bounds, _re_run, dense=True, stores=lambda c: dict(out="f16"))
_case("ray_embed", "C256", (256,), nb=2, Hn=42, Wn=56, h=3, w=4, C=256, eps=1e-5)  # the plans: 462 x 616 -> 33 x 44, C 256 / 512, rows_per_img hw + 4
_case("ray_embed", "C512", (512,), nb=1, Hn=70, Wn=98, h=5, w=7, C=512, eps=1e-5)
_case("ray_embed", "C100", (100,), nb=2, Hn=28, Wn=28, h=4, w=4, C=100, eps=1e-5)
_case("ray_embed", "C384", (384,), nb=2, Hn=42, Wn=56, h=3, w=4, C=384, eps=1e-5)   # the ViT-B/14 plans: 518 x 518 -> 37 x 37, C 384 / 768 / ...
# the inputs cannot lower the variance of sine bands (~0.5): eps raised to variance / 100 instead, so that eps matters as it does on a low-variance row
_case("ray_embed", "C256_eps", (256,), nb=2, Hn=42, Wn=56, h=3, w=4, C=256, eps=5e-3)


# ---- V1 SH_EMBED: antialiased resize, F.normalize, 81 real spherical harmonics (degree <= 8), LayerNorm statistics ----
# T_SH: unit 2^-24, absolute error of one harmonic before the LayerNorm; torch fp32 of the recurrences below against fp64 on these cases: 60.7
# (the degree-8 terms multiply (2m - 1)!! ~ 2 10^6 by normalisations ~ 10^-7)
T_SH = 243.0


def _sh_table(d, dt):
    """Real spherical harmonics Y_l^m(d), l <= 8, of unit vectors d [..., 3] in the order index l (l + 1) + m: the closed forms
    Y_l^m = N_l^|m| P_l^|m|(z) {sqrt2 cos(m phi), 1, sqrt2 sin(|m| phi)} with (x + i y)^m = sin^m(theta) e^{i m phi}, i.e. Cartesian
    polynomials, with the Condon-Shortley phase (-1)^m on both signs of m as utils/sht.py tabulates them: Y_1 = c (-y, z, -x)."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    A, Bm = [torch.ones_like(x)], [torch.zeros_like(x)]
    for m in range(1, 9):
        A.append(A[-1] * x - Bm[-1] * y)
        Bm.append(A[-2] * y + Bm[-1] * x)
    out = [None] * 81
    for m in range(9):
        pmm = float(math.prod(range(2 * m - 1, 0, -2)))                      # (2m - 1)!!: P_m^m / sin^m without the phase
        p2, p1 = None, torch.full_like(z, pmm)
        for l in range(m, 9):
            if l == m:
                p = p1
            elif l == m + 1:
                p = (2 * m + 1) * z * p1
            else:
                p = ((2 * l - 1) * z * p1 - (l + m - 1) * p2) / (l - m)
            if l > m:
                p2, p1 = p1, p
            n = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            if m == 0:
                out[l * (l + 1)] = n * p
            else:
                sgn = (-1.0) ** m * math.sqrt(2.0) * n
                out[l * (l + 1) + m] = sgn * p * A[m]
                out[l * (l + 1) - m] = sgn * p * Bm[m]
    return torch.stack(out, -1)


def _sh_dirs(c, x, dt):
    nb, h, w = c["nb"], c["h"], c["w"]
    t = F.interpolate(x["rays"].to(dt), size=(h, w), mode="bilinear", align_corners=False, antialias=True) if (c["Hn"], c["Wn"]) != (h, w) else x["rays"].to(dt)
    return F.normalize(t.reshape(nb, 3, h * w).permute(0, 2, 1), dim=-1)


def _sh_make(c):
    return dict(rays=_re_rays(c))


def _sh_eval(c, x, dt, eps_scale=1.0):
    return dict(out=_ln(_sh_table(_sh_dirs(c, x, dt), dt), c["eps"] * eps_scale))


def _sh_bounds(c, x, ref):
    return dict(out=_ln_bound(_sh_table(_sh_dirs(c, x, F64), F64), torch.full((), T_SH * U24, dtype=F64), c["eps"]))


def _sh_run(ops, c, x, strided):
    nb, h, w = c["nb"], c["h"], c["w"]
    rpi, ldo = (h * w + 3, 128 + c.get("opad", 40)) if strided else (h * w, 128)
    rows = (torch.arange(nb)[:, None] * rpi + torch.arange(h * w)[None]).reshape(-1)
    go = lg.guarded(nb * rpi, 81, ldo, F16, offset_cols=8 if strided else 0, rows_inside=_dev(rows))    # columns 81.. keep what they hold
    _v1(ops, K_SH_EMBED, a=_flat_in(_dev(x["rays"])), out=go.view, i=(nb, c["Hn"], c["Wn"], h, w, ldo, rpi), f=(c["eps"],))
    return dict(out=go.view[_dev(rows)].view(nb, h * w, 81)), [go]


OPS["sh_embed"] = Op(_sh_make, _sh_eval, _sh_bounds, _sh_run, dense=True, stores=lambda c: dict(out="f16"))
def _sh_form(nb, Hn, Wn, h, w):
    """The footprint form ud_v1_op picks (v1dec.hip): "own", every lane averaging its own token's footprint, or "tpw" with the tokens-per-wave
    bucket -- 1: a wave reduces one token's footprint; "many": it walks 2 .. 64 tokens and lane j keeps token j's direction."""
    ntok = nb * h * w
    if Hn * Wn <= 16 * h * w:
        return ("own",)
    tpw = 64
    while tpw > 1 and ntok // tpw < 4096:
        tpw >>= 1
    return ("tpw", 1 if tpw == 1 else "many")


def _sh_case(id, **kw):
    _case("sh_embed", id, _sh_form(kw["nb"], kw["Hn"], kw["Wn"], kw["h"], kw["w"]), **kw)


# the plans at 462 x 616: -> 132 x 176 (own), -> 112 x 152 (4 tokens per wave), -> 66 x 88 ... 28 x 38 (1 token per wave), ldo 128
_sh_case("own", nb=2, Hn=44, Wn=60, h=11, w=15, eps=1e-5)
_sh_case("tpw", nb=2, Hn=44, Wn=60, h=5, w=7, eps=1e-5)
_sh_case("tpw_ld_odd", nb=1, Hn=64, Wn=64, h=3, w=3, eps=1e-5, opad=41)          # ldo % 8 != 0: the 2-byte store path
_sh_case("tpw_eps", nb=2, Hn=44, Wn=60, h=5, w=7, eps=7e-4)      # the 81 harmonics' variance is ~0.07 whatever the ray: eps = variance / 100
_sh_case("own_many", nb=1, Hn=90, Wn=120, h=45, w=60, eps=1e-5)                  # more than one wave of tokens, a partial last wave
_sh_case("tpw2_partial", nb=1, Hn=370, Wn=370, h=91, w=91, eps=1e-5)             # 8281 tokens: 2 per wave, the last wave holds one
_sh_case("tpw4_partial", nb=1, Hn=520, Wn=520, h=127, w=131, eps=1e-5)           # 16637 tokens: 4 per wave (the plan's count), the last wave holds one
assert [c["cls"][1:] for c in POINTWISE_CASES[-7:]] == [("own",), ("tpw", 1), ("tpw", 1), ("tpw", 1), ("own",), ("tpw", "many"), ("tpw", "many")]


# ======================================================================================================================================
# coverage classes of recorded descriptors (tests/test_layout_coverage_cpu.py)
# ======================================================================================================================================
REQUIRED_CLASSES = {("finalize", 0), ("finalize", 1), ("upsample2x", 1, "shuffle"), ("upsample2x", 1, "lds_wide"), ("ln_patchify2", 4), ("ln_patchify2", 8),
                    ("softmax", "reg20", 0), ("softmax", "generic", 1), ("sh_embed", "tpw", 1), ("sh_embed", "tpw", "many"), ("sh_embed", "own")}
# entry points that other modules hold to the same regime (test_kernel_layouts_gpu.py) or that the issue leaves to per-camera tests; any
# other entry point a plan starts to record (row_stats_finalize: none does today) has no class below and fails point_class by name
ELSEWHERE = {"gemm", "layernorm", "attention", "linear_f32", "camera_head", "preprocess", "rays_camera"}


def point_class(name, a):
    """The coverage class of one recorded `ud_program_add_<name>` call; `a`: its arguments behind the program handle (a descriptor struct
    or the scalar list).  Mirrors the `cls` the cases above declare."""
    if name == "fill_rows":
        return ("fill_rows",)
    if name == "camera_intrinsics":
        return ("camera_intrinsics", a[1] > 1)
    if name == "rays":
        return ("rays", a[5])
    if name == "max":
        return ("max", int(bool(a[3])))
    if name == "spatial_mean":
        return ("spatial_mean", a[4] > 256)
    if name == "nhwc_to_nchw":
        return ("nhwc_to_nchw",)
    if name == "layernorm_patchify2":
        Cc = a[5]
        return ("ln_patchify2", 1 if Cc <= 256 else 2 if Cc <= 512 else 4 if Cc <= 1024 else 8)
    if name == "patchify4":
        return ("patchify4",)
    if name == "attention_small_f32":
        return ("attention_small",)
    d = a[0]
    if name == "upsample2x":
        return ("upsample2x", d.mode, _up_path(d.mode, d.C, d.ldy))
    if name == "resize_ac":
        return ("resize_ac", d.G > 1)
    if name == "finalize":
        return ("finalize", d.mode)
    if name == "ray_embed":
        return ("ray_embed", d.C)
    if name == "dwconv7":
        return ("dwconv7",) + _dw_class(d.C, d.y, d.y16, d.stats_final)
    assert name == "v1_op", name
    i, k = d.i, d.kind
    if k == K_RESIZE_AA:
        return ("resize_aa", "up" if i[3] >= i[10] else "down", (i[8], i[9], i[10], i[11]) != (0, 0, i[1], i[2]), i[5] > 4)
    if k == K_SH_EMBED:
        return ("sh_embed",) + _sh_form(i[0], i[1], i[2], i[3], i[4])
    if k == K_SOFTMAX:
        return ("softmax", _sm_kernel(i[1], i[2], i[3], i[4]), i[4], i[1] > 5120)
    if k == K_ATTN_FEWQ:
        return ("attn_fewq", int(bool(d.c)))
    if k == K_HEAD_MIX:
        return ("head_mix", i[1])
    if k == K_COPY_ROWS:
        return ("copy_rows", i[6], i[3] > 0)
    if k == K_VIT_TAP:
        return ("vit_tap", i[4], int(bool(d.out2)))
    if k == K_RESIZE_AC_SPLIT:
        return ("resize_ac_split", i[5])
    if k == K_PREPROCESS:
        return ("preprocess_v1", i[9], i[10], i[11])
    if k == K_OUT_CONV3:
        return ("out_conv3", i[3])
    return ({K_ADD: "add", K_CAMERA: "camera_v1", K_POINTS: "points", K_MEAN3: "mean3"}[k],)


def class_covered(cls, declared):
    """A recorded class is covered by a declared class that agrees on the op and on every flag the recorded one carries."""
    return any(d[:len(cls)] == cls for d in declared)


# ======================================================================================================================================
# the GPU test
# ======================================================================================================================================
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unidepth_amd import ops as _ops
    return _ops


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def reference(case):
    """(inputs, fp64 reference outputs, bounds, arithmetic part of the bounds) of a case, all on the host."""
    op = OPS[case["op"]]
    x = op.make(case)
    ref = op.evaluate(case, x, F64)
    arith = op.bounds(case, x, ref)
    st = op.stores(case)
    full = {k: (b.double() + term_store(st[k], ref[k]) if k in st else b.double()) for k, b in arith.items()}
    return x, ref, full, arith


@pytest.mark.parametrize("case", POINTWISE_CASES, ids=[c["id"] for c in POINTWISE_CASES])
def test_pointwise_layouts(ops, case):
    """Every case at the strided / offset / guarded layout (and at the dense product layout where the C-ABI has strides): each element of
    each output inside its bound, every guard element intact, and both layouts bit-identical.  Prints the worst error / bound per output."""
    op = OPS[case["op"]]
    x, ref, bnd, _ = reference(case)
    first = None
    for strided in ((False, True) if case.get("dense", op.dense) else (True,)):
        out, guards = op.run(ops, case, x, strided)
        torch.cuda.synchronize()
        for k in ref:
            w = lg.assert_bound(out[k], _dev(ref[k]), _dev(bnd[k].double()), name=f"{case['id']} {'strided' if strided else 'dense'} {k}")
            print(f"RATIO {case['op']} {case['id']} {'strided' if strided else 'dense'} {k} {w:.4f}")
        for i, g in enumerate(guards):
            g.check_guards(f"{case['id']} {'strided' if strided else 'dense'} output {i}")
        got = {k: _bits(v).clone() for k, v in out.items()}
        if first is None:
            first = got
        else:
            for k in got:
                assert torch.equal(first[k], got[k]), f"{case['id']}: output {k} differs between the dense and the strided layout"
