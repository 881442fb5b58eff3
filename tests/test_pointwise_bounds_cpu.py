"""The bounds of tests/test_pointwise_layouts_gpu.py, checked on the CPU with no kernel (the style of tests/test_layout_guard_cpu.py):

  headroom     for every GPU case the same inputs, the op evaluated by torch in fp32, passed through the same bound: it must hold with a
               factor of 4 to spare (the margin rule of C_ACC) -- a bound that plain fp32 arithmetic already fills would fail a correct
               kernel whose summation order differs.  The probe is held to the ARITHMETIC part of the bound: the term of an fp16 store
               (2^-11 |ref|, reached by a correct rounding) is a property of the format and is left out on both sides;
  sensitivity  each defect below, planted into the fp64 torch statement, must leave the bound on every case it touches -- a bound loose
               enough to pass one of them would pass a kernel with that defect."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("test_pointwise_layouts_gpu", os.path.join(_here, "test_pointwise_layouts_gpu.py"))
pw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pw)
lg = pw.lg

CASES = pw.POINTWISE_CASES
_ids = [c["id"] for c in CASES]
_cache = {}


def _ref(case):
    if case["id"] not in _cache:
        _cache.clear()                                                        # one case at a time: the second-trip cases are large
        _cache[case["id"]] = pw.reference(case)
    return _cache[case["id"]]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fp32_torch_stays_four_times_inside_the_bound(case):
    x, ref, bnd, arith = _ref(case)
    out = pw.OPS[case["op"]].evaluate(case, x, torch.float32)
    assert set(out) == set(ref) == set(bnd)
    for k in ref:
        assert ref[k].dtype == torch.float64 or arith[k].dim() == 0, (k, ref[k].dtype)     # exact outputs may keep their storage type
        lg.assert_bound(out[k], ref[k], arith[k].double(), name=f"{case['id']} {k}", margin=4.0)


def test_explicit_bilinear_is_torch_interpolate():
    """The gather form the resampling cases use (and plant defects into) is F.interpolate, at both align_corners settings."""
    x = pw._rnd((2, 9, 11, 8), 0).double()
    for ac, (Ho, Wo) in ((False, (18, 22)), (True, (16, 19)), (True, (5, 4)), (False, (23, 30))):
        want = F.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=ac).permute(0, 2, 3, 1)
        got = pw._bilinear(x, Ho, Wo, torch.float64, ac)
        assert (got - want).abs().max() < 1e-13, (ac, Ho, Wo)


@pytest.mark.parametrize("kind,kw", [("aa", dict(mode="bilinear", antialias=True)), ("linear", dict(mode="bilinear")), ("cubic", dict(mode="bicubic"))])
def test_explicit_axis_weights_are_torch_interpolate(kind, kw):
    """The separable weight matrices the resize bounds are built from (mag, the sum of the |tap values|) reproduce F.interpolate, up- and
    down-sampling, and the support covers every non-zero weight."""
    x = pw._rnd((2, 3, 29, 39), 0).double()
    for Ho, Wo in ((7, 10), (58, 77), (29, 40), (30, 13)):
        (Wy, Sy), (Wx, Sx) = pw._axis_weights(kind, Ho, 29), pw._axis_weights(kind, Wo, 39)
        want = F.interpolate(x, size=(Ho, Wo), align_corners=False, **kw)
        assert (pw._separable(x, Wy, Wx) - want).abs().max() < 1e-13, (kind, Ho, Wo)
        assert bool(((Wy != 0) <= (Sy > 0)).all()) and bool(((Wx != 0) <= (Sx > 0)).all())
        assert (Wy.sum(1) - 1).abs().max() < 1e-13


def test_hi_nearest_check_accepts_correct_pairs_and_rejects_a_neighbour():
    """The [hi | lo] check of the GPU module: fp16 splits of fp32 values pass (ties, subnormals, both sides of powers of two included), and
    a hi one grid step off fails -- also just below a power of two, where the grid is twice as fine."""
    v = torch.cat([pw._rnd((200000,), 3, 3.0), torch.tensor([1.0 - 2.0 ** -13, 2.0 - 2.0 ** -12 + 2.0 ** -20, -4.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 6e-6, 0.0])])
    hi = v.half()
    pw._assert_hi_nearest(hi, (v - hi.float()).half(), "exact splits")
    for val, wrong in ((1.0 - 0.75 * 2.0 ** -11, 1.0), (1.0 + 0.75 * 2.0 ** -10, 1.0), (-2.0 + 0.75 * 2.0 ** -10, -2.0)):
        v, hi = torch.tensor([val]), torch.tensor([wrong]).half()
        with pytest.raises(AssertionError):
            pw._assert_hi_nearest(hi, (v - hi.float()).half(), "neighbour")


def test_spherical_harmonics_table_is_orthonormal():
    """The closed forms of the SH_EMBED reference: 81 functions, orthonormal on the sphere (quadrature), Y_0^0 = 1 / sqrt(4 pi), Y_1 = c (-y, z, -x)."""
    n = 64
    zs, ws = [torch.tensor(v, dtype=torch.float64) for v in np.polynomial.legendre.leggauss(n)]
    ph = torch.arange(2 * n, dtype=torch.float64) * (math.pi / n)
    st = torch.sqrt(1 - zs * zs)
    d = torch.stack([st[:, None] * torch.cos(ph)[None], st[:, None] * torch.sin(ph)[None], zs[:, None].expand(n, 2 * n)], -1)
    Y = pw._sh_table(d, torch.float64)
    gram = torch.einsum("zpi,zpj,z->ij", Y, Y, ws) * (math.pi / n)
    assert (gram - torch.eye(81, dtype=torch.float64)).abs().max() < 1e-10
    c1 = math.sqrt(3 / (4 * math.pi))
    assert (Y[..., 0] - 1 / math.sqrt(4 * math.pi)).abs().max() < 1e-15
    assert (Y[..., 1:4] - c1 * d[..., [1, 2, 0]] * torch.tensor([-1.0, 1.0, -1.0], dtype=torch.float64)).abs().max() < 1e-14


# defect -> (keyword planted into Op.evaluate, the cases it touches, dtype it is planted at)
def _is(op, **kw):
    return lambda c: c["op"] in (op if isinstance(op, tuple) else (op,)) and all(c.get(k) == v for k, v in kw.items())


DEFECTS = {
    "align_corners flipped": (dict(flip_align=True), _is(("resize_ac", "resize_ac_split")), torch.float64),
    "half-pixel offset dropped": (dict(half_pixel=False), _is("upsample2x"), torch.float64),
    "neighbour clamp omitted": (dict(clamp=False), _is("upsample2x"), torch.float64),
    "0.25 / 0.75 row weights swapped": (dict(swap_rows=True), _is("upsample2x"), torch.float64),
    "eps x 10": (dict(eps_scale=10.0), lambda c: (c["op"] == "upsample2x" and c["mode"] == 1) or c["op"] in ("ln_patchify2", "ray_embed", "sh_embed")
                 or (c["op"] == "dwconv7" and c.get("final")), torch.float64),
    "one antialias tap 1 % heavy": (dict(tap="heavy"), _is("resize_aa"), torch.float64),
    "one antialias support tap missing": (dict(tap="missing"), _is("resize_aa"), torch.float64),
    "antialias off on a down-sample": (dict(no_antialias=True), lambda c: c["op"] == "resize_aa" and c["cls"][1] == "down", torch.float64),
    "class token not added": (dict(no_cls=True), _is("vit_tap"), torch.float64),
    "lo term dropped": (dict(drop_lo=True), lambda c: c["op"] == "resize_ac_split" or (c["op"] == "copy_rows" and c["to_f16"] == 2), torch.float32),
    "softmax pad columns non-zero": (dict(pad_garbage=True), lambda c: c["op"] == "softmax" and c["ldo"] > c["N"], torch.float64),
    "mean over HW + 1": (dict(hw_plus_one=True), _is("spatial_mean"), torch.float64),
}
def _eps_sensitive(c):
    """eps x 10 is visible where a case holds rows of deviation ~10 sqrt(eps) (or, for the embeddings whose variance the inputs cannot
    lower, an eps raised to their variance): the cases built that way.  On the others eps stays below the fp16 store
    (test_eps_is_invisible_at_unit_variance), so the defect does not touch them."""
    return c["op"] not in ("ray_embed", "sh_embed") or c.get("eps", 0) > 1e-4


_touched = [(name, c) for name, (_, touches, _) in DEFECTS.items() for c in CASES
            if touches(c) and "second_trip" not in c["id"] and (name != "eps x 10" or _eps_sensitive(c))]


@pytest.mark.parametrize("name,case", _touched, ids=[f"{n}|{c['id']}" for n, c in _touched])
def test_planted_defect_leaves_the_bound(name, case):
    kw, _, dt = DEFECTS[name]
    x, ref, bnd, _ = _ref(case)
    bad = pw.OPS[case["op"]].evaluate(case, x, dt, **kw)
    failed = []
    for k in ref:
        try:
            lg.assert_bound(bad[k], ref[k], bnd[k].double(), name=k)
        except AssertionError:
            failed.append(k)
    assert failed, f"{name} passes every bound of {case['id']}"
    if name == "neighbour clamp omitted" and case["mode"] == 0:              # the defect touches the border row / column only, and only they fail
        ratio, _ = lg.bound_ratio(bad["out"], ref["out"], bnd["out"].double())
        inner = ratio[:, :-1, :-1]
        assert float(inner.max()) <= 1.0 and float(ratio[:, -1].max()) > 1.0 and float(ratio[:, :, -1].max()) > 1.0


def test_every_listed_defect_touches_a_case():
    seen = {n for n, _ in _touched}
    assert seen == set(DEFECTS), set(DEFECTS) - seen
    assert {"ray_embed", "sh_embed", "upsample2x", "ln_patchify2", "dwconv7"} <= {c["op"] for n, c in _touched if n == "eps x 10"}


def test_eps_is_invisible_at_unit_variance():
    """Why the LayerNorm-statistic cases carry low-variance rows: on unit-variance rows alone eps x 10 stays inside the fp16 store rounding."""
    c = dict(next(c for c in CASES if c["id"] == "ln_patchify2-C192"))
    x = pw.OPS["ln_patchify2"].make(c)
    x["x"] = pw._rnd(tuple(x["x"].shape), 5) * 1.5 + 0.4
    ref = pw.OPS["ln_patchify2"].evaluate(c, x, torch.float64)
    bnd = pw.OPS["ln_patchify2"].bounds(c, x, ref)["out"].double() + pw.term_store("f16", ref["out"])
    bad = pw.OPS["ln_patchify2"].evaluate(c, x, torch.float64, eps_scale=10.0)
    lg.assert_bound(bad["out"], ref["out"], bnd)
