"""Golden vectors of the colourising (unidepth_amd/visualization.py): the reference's own colorize and image_grid
(unidepth/utils/visualization.py: numpy + matplotlib + PIL on the CPU) on seeded inputs -> tests/golden/colorize.npz.

    python tools/make_golden_colorize.py          (needs the reference tree, matplotlib and PIL; only output bytes are written)

This module also holds what the tests share: CASES / case_inputs(name) (seeded CPU torch.Generator inputs, rebuilt on any machine),
arel() and restate() -- an independent numpy restatement of ud_colorize's per-pixel arithmetic (include/unidepth_hip.h UdColorize) in
fp32, every operation rounded separately -- and restate_grid().  The golden file also carries the LUT rows that the reference used
(lut_<name>), so the tests need no matplotlib.  Nothing from the reference is imported at module import time."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "colorize.npz")
REF_VIS = os.path.join("unidepth", "utils", "visualization.py")

F32 = np.float32
INVALID = 1e-4                                   # the reference's invalid threshold
BELOW_INVALID = np.nextafter(F32(INVALID), F32(0))

# name -> (kind, H, W, vmin, vmax, cmap); kind selects the generator in case_inputs
CASES = {
    "both_magma_r":      ("uniform", 24, 31, 0.01, 10.0, "magma_r"),
    "both_coolwarm":     ("uniform", 24, 31, 0.0, 0.2, "coolwarm"),
    "lo_magma_r":        ("uniform", 23, 32, 0.5, None, "magma_r"),
    "hi_coolwarm":       ("uniform", 23, 32, None, 5.0, "coolwarm"),
    "lo_coolwarm":       ("uniform", 7, 13, 0.5, None, "coolwarm"),
    "hi_magma_r":        ("uniform", 7, 13, None, 5.0, "magma_r"),
    "none_magma_r":      ("uniform", 25, 30, None, None, "magma_r"),
    "none_coolwarm":     ("uniform", 25, 30, None, None, "coolwarm"),
    "f64_both_magma_r":  ("f64", 24, 31, 0.01, 10.0, "magma_r"),
    "edges_magma_r":     ("edges", 3, 257, 0.01, 10.0, "magma_r"),
    "edges_coolwarm":    ("edges", 3, 257, 0.0, 0.2, "coolwarm"),
    "special_magma_r":   ("special", 3, 8, 0.01, 10.0, "magma_r"),
    "special_coolwarm":  ("special", 3, 8, -1.0, 10.0, "coolwarm"),
    "nan_auto":          ("nan", 5, 9, None, None, "magma_r"),
    "nan_auto_hi":       ("nan", 5, 9, 0.01, None, "magma_r"),
    "const_auto":        ("const", 5, 9, None, None, "magma_r"),
    "posinf_auto":       ("posinf", 5, 9, None, None, "coolwarm"),
    "neginf_auto":       ("neginf", 5, 9, None, None, "coolwarm"),
    "arel_coolwarm":     ("arel", 24, 31, 0.0, 0.2, "coolwarm"),
}
# image_grid cases: name -> (rows, cols, the colorize cases whose reference outputs are the images; "rgb" = case_rgb())
GRIDS = {
    "grid_2x2": (2, 2, ("rgb", "f64_both_magma_r", "both_magma_r", "arel_coolwarm")),
    "grid_1x2": (1, 2, ("rgb", "both_magma_r")),
}
GRID_HW = (24, 31)


def _uniform(name, H, W, lo, hi):
    """fp32 [H,W], uniform draws and ONE multiply-add only: exp / log / randn round differently from one CPU's vector library to the
    next, and the golden bytes depend on every bit of the input."""
    g = torch.Generator().manual_seed(3000 + sorted(CASES).index(name))
    return (lo + (hi - lo) * torch.rand(H, W, generator=g)).float().numpy()


def arel(g, p):
    """The demo's error map from fp32 g, p: |g - p| / g with every operation rounded to fp32, 0 where g == 0."""
    g, p = np.asarray(g, F32), np.asarray(p, F32)
    with np.errstate(all="ignore"):
        e = (np.abs(g - p) / g).astype(F32)
    e[g == 0.0] = 0.0
    return e


def arel_inputs(name="arel_coolwarm"):
    """(g, p) fp32 of the error-map case: g has zeros (no ground truth), p scatters around g by up to ~25 %."""
    _, H, W, _, _, _ = CASES[name]
    g = _uniform(name, H, W, 0.5, 8.0)
    gen = torch.Generator().manual_seed(4000)
    p = (torch.from_numpy(g) * (0.75 + 0.5 * torch.rand(H, W, generator=gen))).float().numpy()
    g[::5, ::3] = 0.0
    g[3, 4] = p[3, 4]                                          # an exact zero error
    return g, p


def case_rgb():
    """uint8 [H,W,3] image of the grid cases."""
    g = torch.Generator().manual_seed(4100)
    return torch.randint(0, 256, (*GRID_HW, 3), generator=g, dtype=torch.uint8).numpy()


def case_inputs(name):
    """The value array of a golden case: fp32 [H,W] (float64 for the f64 case)."""
    kind, H, W, vmin, vmax, _ = CASES[name]
    if kind == "uniform":
        lo = -0.1 if vmin is None else vmin - 0.2 * ((vmax if vmax is not None else vmin + 10.0) - vmin)
        hi = (vmax if vmax is not None else (vmin if vmin is not None else 0.0) + 10.0)
        hi = hi + 0.2 * (hi - lo)
        return _uniform(name, H, W, lo, hi)
    if kind == "f64":                                          # demo.py's ground truth: uint16 millimetres .astype(float) / 1000.0
        g = torch.Generator().manual_seed(3000 + sorted(CASES).index(name))
        mm = torch.randint(0, 12000, (H, W), generator=g).numpy()
        mm[::4, ::7] = 0
        return mm.astype(float) / 1000.0
    if kind == "edges":                                        # exact bin edges vmin + (vmax - vmin) k / 256 and their fp32 neighbours
        k = np.arange(257, dtype=np.float64)
        e = (vmin + (vmax - vmin) * k / 256.0).astype(F32)
        return np.stack([e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))]).astype(F32)
    if kind == "special":
        v = np.array([vmax, np.nextafter(F32(vmax), F32(np.inf)), np.nextafter(F32(vmax), F32(0)), 2 * vmax + 1, 1e30, vmin, vmin - 0.5, -3.0,
                      INVALID, BELOW_INVALID, np.nextafter(F32(INVALID), F32(1)), 0.0, -0.0, 1e-30, -1e-30, 5e-5,
                      np.nan, np.inf, -np.inf, 0.5 * (vmin + vmax), 1.0, 2.0, 9.999, -1.0], dtype=F32)
        return v.reshape(H, W)
    v = _uniform(name, H, W, 0.5, 6.0)
    if kind == "nan":
        v[2, 3] = np.nan
    elif kind == "const":
        v[:] = 2.5
    elif kind == "posinf":
        v[1, 1] = np.inf
    elif kind == "neginf":
        v[1, 1] = -np.inf
    elif kind == "arel":
        return arel(*arel_inputs(name))
    return v


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def restate(value, lut, vmin=None, vmax=None, dtype=F32):
    """ud_colorize's per-pixel arithmetic restated on one image: value [H,W], lut uint8 [256,3], Python-float limits or None (the image's
    own minimum / maximum) -> uint8 [H,W,3].  `dtype` is the precision of every operation (fp32 = the kernel; float64 = the host path
    on a float64 array)."""
    T = dtype
    v = np.asarray(value).astype(T)
    lut = np.asarray(lut)
    assert v.ndim == 2 and lut.shape == (256, 3) and lut.dtype == np.uint8
    with np.errstate(all="ignore"):
        invalid = v < T(INVALID)                                               # false for a NaN
        if vmin is not None and vmax is not None:
            lo, den = T(vmin), T(float(vmax) - float(vmin))                    # the difference in double, then rounded
        else:
            lo = v.min() if vmin is None else T(vmin)                          # NaN if any pixel is NaN
            hi = v.max() if vmax is None else T(vmax)
            den = T(hi - lo)
        t = ((v - lo).astype(T) / den).astype(T)
        x = (t * T(256)).astype(T)
        nan = np.isnan(x)
        idx = np.where(nan, 0, np.where(x < 0, 0, np.where(x >= 256, 255, x))).astype(np.int64)      # truncation of [0, 256)
    out = lut[idx]
    out[nan | invalid] = 0
    return out


def restate_grid(cells, rows, cols):
    """rows * cols equal-sized uint8 [H,W,3] images (None = a cell left alone, filled with zeros here) pasted row-major."""
    H, W = next(c for c in cells if c is not None).shape[:2]
    grid = np.zeros((rows * H, cols * W, 3), dtype=np.uint8)
    for i, c in enumerate(cells):
        if c is not None:
            grid[i // cols * H:(i // cols + 1) * H, i % cols * W:(i % cols + 1) * W] = c
    return grid


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_path():
    """visualization.py in the reference tree (oracle/ref_loader.py REF_ROOT; present on the authoring machine only)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return os.path.join(ref_loader.REF_ROOT, REF_VIS)


def reference_module():
    """The reference's visualization module, loaded from the reference tree with stand-ins for wandb and unidepth.utils.misc (neither is
    used by colorize / image_grid); matplotlib and PIL are the real ones."""
    import importlib.util
    names = ("wandb", "unidepth", "unidepth.utils", "unidepth.utils.misc")
    saved = {k: sys.modules.get(k) for k in names}
    for k in names:
        sys.modules[k] = types.ModuleType(k)
    sys.modules["unidepth.utils.misc"].ssi_helper = None
    try:
        spec = importlib.util.spec_from_file_location("_ref_visualization", reference_path())
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def reference_outputs(mod):
    """name -> the reference's bytes for every colorize case, every grid case, and the LUT rows of the colormaps the cases use."""
    import matplotlib.pyplot as plt
    out = {}
    for name, (_, H, W, vmin, vmax, cmap) in CASES.items():
        with np.errstate(all="ignore"):
            img = np.asarray(mod.colorize(case_inputs(name), vmin=vmin, vmax=vmax, cmap=cmap))
        assert img.dtype == np.uint8 and img.shape == (H, W, 3), (name, img.dtype, img.shape)
        out[name] = np.ascontiguousarray(img)
    for name, (rows, cols, cells) in GRIDS.items():
        grid = np.asarray(mod.image_grid([case_rgb() if c == "rgb" else out[c] for c in cells], rows, cols))
        assert grid.dtype == np.uint8 and grid.shape == (rows * GRID_HW[0], cols * GRID_HW[1], 3), (name, grid.shape)
        out[name] = grid
    for cmap in sorted({c[5] for c in CASES.values()}):
        out["lut_" + cmap] = np.ascontiguousarray(plt.get_cmap(cmap)(np.arange(256), bytes=True)[:, :3])
    return out


def main():
    out = reference_outputs(reference_module())
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
