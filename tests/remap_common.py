"""What the remap tests share (not a test module): the numpy restatements and seeded inputs of tools/make_golden_remap.py, the input sets
both the host build and the GPU run are compared on, each set's restatement computed once per process, and the measured bars of
tests/golden/remap.npz."""
import functools
import importlib.util
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_remap", os.path.join(ROOT, "tools", "make_golden_remap.py"))
rm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rm)
up, gp, cp = rm.up, rm.gp, rm.cp

# (mode, padding, normalize, src_mask present, coord_valid present): all 32
CONFIGS = tuple(itertools.product(rm.MODES, rm.PADDINGS, (False, True), (False, True), (False, True)))

# name -> (Hs, Ws, C, B, uint8 source, source batch, uv batch, mask batch, points)
#   points: ("regular", N) seeded draws up to a quarter of the image outside it, followed by the special coordinates;
#           "centres" the materialised pixel centres (48 * 64 = 3072 points: 12 workgroups per image)
SETS = {
    "f32_37x53_c3_b3": (37, 53, 3, 3, False, 3, 3, 3, ("regular", 257)),
    "u8_48x64_c5_b1": (48, 64, 5, 1, True, 1, 1, 1, ("regular", 255)),
    "f32_48x64_c1_b3_shared_uv": (48, 64, 1, 3, False, 3, 1, 3, "centres"),
    "u8_37x53_c3_b3_shared_src": (37, 53, 3, 3, True, 1, 3, 1, ("regular", 65)),
    "f32_37x53_c5_b1_centres": (37, 53, 5, 1, False, 1, 1, 1, "centres"),
}
POINT_COUNTS = (1, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(src, uv [uvB,N,2], mask uint8 [maskB,Hs,Ws], cv uint8 [B,N], B, n_regular) of a set; read-only"""
    Hs, Ws, C, B, u8, sb, ub, mb, pts = SETS[name]
    k = sorted(SETS).index(name)
    src = rm.source(Hs, Ws, C, sb, 7500 + k, u8=u8)
    if pts == "centres":
        uv, n_reg = rm.centre_points(Hs, Ws), 0
        assert ub == 1
    else:
        reg, sp = rm.regular_points(Hs, Ws, ub, pts[1], 7600 + k), rm.special_points(Hs, Ws)
        uv, n_reg = np.concatenate([reg, np.repeat(sp, ub, axis=0)], axis=1), pts[1]
    d = dict(src=src, uv=np.ascontiguousarray(uv), mask=rm.source_mask(Hs, Ws, mb, 7700 + k), cv=rm.coord_valid(B, uv.shape[1], 7800 + k),
             B=B, n_regular=n_reg)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def want(name, cfg, out_u8=False, n=None):
    """the fp32 restatement (out [B,N,C], valid [B,N]) of a set under a configuration, on its first n points"""
    mode, padding, normalize, has_mask, has_cv = cfg
    d = inputs(name)
    n = d["uv"].shape[1] if n is None else n
    return rm.remap(d["src"], d["uv"][:, :n], mode, padding, d["mask"] if has_mask else None, d["cv"][:, :n] if has_cv else None, normalize, out_u8)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(rm.GOLDEN))


def bars():
    g = golden()
    return {k: rm.bar(float(g["referr." + k])) for k in rm.MODES + ("undistort",)}


def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


def same_bits(a, b):
    """bit for bit, the sign of a zero included; a NaN equals a NaN whatever its sign and payload"""
    if a.dtype != np.float32:
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def overlap_fields():
    """name -> uv fp32 [B,2,H,W]: the synthetic fields from their formulas, the projected ones from the golden file"""
    g = golden()
    out = {name: rm.overlap_field(name) for name in rm.OV_FIELDS}
    out.update({"proj_" + name: g["proj_" + name + ".uv"] for name in rm.OV_PROJECTED})
    return out
