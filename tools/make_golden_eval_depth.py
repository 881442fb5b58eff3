"""Golden vectors of the 2-D depth metrics (unidepth_amd/eval_ops.py eval_depth): the reference's own eval_depth
(unidepth/utils/evaluation_depth.py, run on the CPU) on seeded inputs -> tests/golden/eval_depth.npz.

    python tools/make_golden_eval_depth.py          (needs the reference tree; only its outputs are written)

This module also holds what the tests share: CASES / case_inputs(name) (seeded CPU torch.Generator inputs, rebuilt on any machine),
restate() -- an independent numpy restatement of the metric definitions (fp32 where the definition computes in fp32, fp64 sums) that
the GPU tests use at sizes too large for a golden file -- and compare(), the tolerance rule.  Nothing from the reference is imported at
module import time."""
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_depth.npz")
REF_EVAL = os.path.join("unidepth", "utils", "evaluation_depth.py")

KEYS = ("d1_ssi", "d1_si", "d1", "d2", "d3", "rmse", "rmselog", "arel_ssi", "arel_si", "arel", "sqrel", "log10", "silog",
        "medianlog", "d_auc", "tau_ssi", "tau_si", "tau")
COUNT_KEYS = ("d1", "d2", "d3", "tau", "d_auc")
RESCALED_COUNT_KEYS = ("d1_ssi", "d1_si", "tau_ssi", "tau_si")
MEAN_KEYS = ("rmse", "rmselog", "arel_ssi", "arel_si", "arel", "sqrel", "log10", "silog")

# name -> (B, (H, W), (h, w), mask kind, max_depth)
CASES = {
    "equal_b2_60x80": (2, (60, 80), (60, 80), "dense", None),
    "up_b2_120x160_from_37x53_maxd": (2, (120, 160), (37, 53), "dense", 12.0),
    "down_b2_48x64_from_101x131": (2, (48, 64), (101, 131), "dense", None),
    "sparse_b2_75x248_from_56x186": (2, (75, 248), (56, 186), "sparse", None),
    "ties_b2_int_40x50": (2, (40, 50), (40, 50), "ties", None),
    "edge_b3_empty_zero_two": (3, (32, 40), (32, 40), "edge", None),
}


def random_inputs(g: torch.Generator, B, HW, hw, mask_kind, max_depth=None):
    """gts [B,1,H,W], preds [B,1,h,w], masks [B,1,H,W] bool: a smooth positive prediction, a ground truth that follows it with
    log-normal noise (ratios spread over every threshold), and a dense (~85 %) or sparse LiDAR-like (~10 %) validity mask."""
    (H, W), (h, w) = HW, hw
    base = torch.exp(torch.randn(B, 1, max(2, h // 8), max(2, w // 8), generator=g) * 0.6 + 1.5)
    pred = F.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)
    pred = pred * torch.exp(0.05 * torch.randn(B, 1, h, w, generator=g))
    up = F.interpolate(pred, size=(H, W), mode="bilinear", align_corners=False)
    gt = up * 1.1 * torch.exp(0.25 * torch.randn(B, 1, H, W, generator=g))
    frac = 0.1 if mask_kind == "sparse" else 0.85
    masks = torch.rand(B, 1, H, W, generator=g) < frac
    return gt.float(), pred.float(), masks


def case_inputs(name):
    """(gts, preds, masks, max_depth) of a golden case, on the CPU."""
    B, HW, hw, kind, max_depth = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    (H, W), (h, w) = HW, hw
    if kind == "ties":
        # integer depths: many equal values (median ties) and ratios exactly 1.25 = 5/4 = 10/8
        gt = torch.randint(1, 11, (B, 1, H, W), generator=g).float()
        pred = torch.randint(1, 11, (B, 1, h, w), generator=g).float()
        pred[:, :, ::3] = gt[:, :, ::3] * 1.25
        pred[:, :, 1::7] = gt[:, :, 1::7] / 1.25
        masks = torch.rand(B, 1, H, W, generator=g) < 0.9
        return gt, pred, masks, max_depth
    gt, pred, masks = random_inputs(g, B, HW, hw, "sparse" if kind == "sparse" else "dense")
    if kind == "edge":
        masks[0] = False                                    # no valid pixel: every metric NaN
        zs = torch.nonzero(masks[1, 0])[:5]
        pred[1, 0, zs[:, 0], zs[:, 1]] = 0.0                # a few p = 0 inside V: inf / NaN where the definitions give them
        masks[2] = False
        masks[2, 0, 3, 7] = True                            # two valid pixels
        masks[2, 0, 20, 31] = True
    return gt, pred, masks, max_depth


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _f32(x):
    return np.float32(x)


def resample(pred: np.ndarray, H: int, W: int) -> np.ndarray:
    """Bilinear [h,w] -> [H,W] as F.interpolate(mode="bilinear", align_corners=False): src = scale (dst + 0.5) - 0.5 clamped at 0,
    index = min(floor(src), size - 1), lambda = clamp(src - index, 0, 1), scale = size_in / size_out, all in fp32;
    out = (v00 w0x + v01 w1x) w0y + (v10 w0x + v11 w1x) w1y, every operation rounded to fp32.  Identity when the shapes agree."""
    h, w = pred.shape
    if (h, w) == (H, W):
        return pred.astype(np.float32)

    def axis(n_in, n_out):
        sc = _f32(n_in) / _f32(n_out)
        f = sc * (np.arange(n_out, dtype=np.float32) + _f32(0.5)) - _f32(0.5)
        f = np.maximum(f, _f32(0.0))
        i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
        lam = np.clip(f - i0.astype(np.float32), _f32(0.0), _f32(1.0)).astype(np.float32)
        i1 = i0 + (i0 < n_in - 1)
        return i0, i1, (_f32(1.0) - lam).astype(np.float32), lam

    y0, y1, hy, ly = axis(h, H)
    x0, x1, hx, lx = axis(w, W)
    p = pred.astype(np.float32)
    t0 = p[y0][:, x0] * hx + p[y0][:, x1] * lx
    t1 = p[y1][:, x0] * hx + p[y1][:, x1] * lx
    return (t0 * hy[:, None] + t1 * ly[:, None]).astype(np.float32)


def _ratio(g, p):
    return np.maximum(g / p, p / g)               # np.maximum propagates NaN, as torch.maximum


def _lower_median(x):
    if x.size == 0 or np.isnan(x).any():
        return np.float32(np.nan)
    return np.sort(x)[(x.size - 1) // 2]


def dauc_thresholds():
    """(1.25 ** e, e) for e = linspace(0.01, 5.0, 100), fp32, as torch makes them."""
    e = torch.linspace(0.01, 5.0, steps=100)
    return (1.25 ** e).numpy(), e.numpy()


def restate_one(g: np.ndarray, p: np.ndarray, thr=None) -> dict:
    """The 18 metrics of the valid pixels g, p (1-D fp32) of one image; fp32 per-element values, fp64 sums."""
    thr_e = thr if thr is not None else dauc_thresholds()
    n = g.size
    if n == 0:
        return {k: np.nan for k in KEYS}
    with np.errstate(all="ignore"):
        r = _ratio(g, p)
        lg, lp = np.log(g), np.log(p)
        d = lp - lg
        e = g - p
        m = {}
        frac = lambda mask: float(np.float32(np.count_nonzero(mask)) / np.float32(n))
        m["d1"], m["d2"], m["d3"] = frac(r < _f32(1.25)), frac(r < _f32(1.5625)), frac(r < _f32(1.953125))
        m["tau"] = frac(r < _f32(1.03))
        m["rmse"] = math.sqrt(np.sum((e * e).astype(np.float64)) / n)
        m["rmselog"] = math.sqrt(np.sum(((lg - lp) ** 2).astype(np.float64)) / n)
        m["arel"] = float(np.sum((np.abs(e) / g).astype(np.float64)) / n)
        m["sqrel"] = float(np.sum(((e * e) / g).astype(np.float64)) / n)
        m["log10"] = float(np.sum(np.abs(np.log10(p) - np.log10(g)).astype(np.float64)) / n)
        d64 = d.astype(np.float64)
        m["silog"] = 100.0 * math.sqrt(np.sum((d64 - d64.mean()) ** 2) / (n - 1)) if n > 1 else np.nan
        m["medianlog"] = float(np.float32(100.0) * np.abs(_lower_median(d)))
        fr = np.array([np.float32(np.count_nonzero(r < t)) / np.float32(n) for t in thr_e[0]], dtype=np.float64)
        ex = thr_e[1].astype(np.float64)
        m["d_auc"] = float(np.sum((ex[1:] - ex[:-1]) * (fr[1:] + fr[:-1])) / 2.0 / 5.0)
        # si: p * med(g) / med(p), fp32, multiply first
        psi = (p * _lower_median(g)).astype(np.float32) / _lower_median(p)
        # ssi: ([[sum p^2, sum p], [sum p, n]] + 1e-9 I) [s, t] = [sum p g, sum g] in fp64; p'' = s p + t in fp32
        p64, g64 = p.astype(np.float64), g.astype(np.float64)
        A = np.array([[np.sum(p64 * p64) + 1e-9, np.sum(p64)], [np.sum(p64), n + 1e-9]])
        rhs = np.array([np.sum(p64 * g64), np.sum(g64)])
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        s = (A[1, 1] * rhs[0] - A[0, 1] * rhs[1]) / det
        t = (A[0, 0] * rhs[1] - A[1, 0] * rhs[0]) / det
        pssi = (p * _f32(s)).astype(np.float32) + _f32(t)
        for tag, q in (("ssi", pssi), ("si", psi)):
            rq = _ratio(g, q)
            m[f"d1_{tag}"] = frac(rq < _f32(1.25))
            m[f"tau_{tag}"] = frac(rq < _f32(1.03))
            m[f"arel_{tag}"] = float(np.sum((np.abs(g - q) / g).astype(np.float64)) / n)
    return {k: m[k] for k in KEYS}


def restate(gts, preds, masks, max_depth=None):
    """eval_depth restated per image -> ({key: fp64 [B]}, n [B]).  Accepts CPU torch tensors or numpy arrays shaped [B,1,*,*]."""
    gts, preds, masks = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (gts, preds, masks))
    B, _, H, W = gts.shape
    thr = dauc_thresholds()
    out = {k: np.zeros(B) for k in KEYS}
    ns = np.zeros(B, dtype=np.int64)
    for b in range(B):
        g = gts[b, 0].astype(np.float32)
        p = resample(preds[b, 0], H, W)
        v = masks[b, 0].astype(bool)
        if max_depth is not None:
            v = v & (g <= np.float32(max_depth))
        ns[b] = int(v.sum())
        for k, val in restate_one(g[v], p[v], thr).items():
            out[k][b] = val
    return out, ns


def compare(got: dict, ref: dict, ns) -> list:
    """Tolerance rule between two metric dicts ({key: [B]}) for images with n valid pixels: the same finite / +-inf / NaN pattern, then
    unrescaled counting metrics |diff| n <= 2, rescaled ones |diff| n <= max(3, 1e-4 n), means and silog relative 1e-5 (arel_ssi: or
    2e-6 absolute), medianlog 1e-4 absolute.  Returns the failures (empty = agree)."""
    bad = []
    for k in KEYS:
        a = np.asarray(got[k], dtype=np.float64)
        b = np.asarray(ref[k], dtype=np.float64)
        for i in range(b.size):
            x, y, n = a[i], b[i], int(ns[i])
            if np.isnan(x) or np.isnan(y) or np.isinf(x) or np.isinf(y):
                if not (np.isnan(x) and np.isnan(y)) and x != y:
                    bad.append(f"{k}[{i}]: {x} vs {y} (non-finite pattern)")
                continue
            if k in COUNT_KEYS:
                ok = abs(x - y) * n <= 2.0 + 1e-6
            elif k in RESCALED_COUNT_KEYS:
                ok = abs(x - y) * n <= max(3.0, 1e-4 * n) + 1e-6
            elif k == "medianlog":
                ok = abs(x - y) <= 1e-4
            elif k == "arel_ssi":
                # the reference solves the ssi system from fp32 sums: its fit is off by fp32 noise, which is all of the value when
                # the fit is exact (two valid pixels: arel_ssi = 0 in exact arithmetic, ~5e-7 in the reference)
                ok = abs(x - y) <= max(1e-5 * abs(y), 2e-6)
            else:
                ok = abs(x - y) <= 1e-5 * abs(y)
            if not ok:
                bad.append(f"{k}[{i}]: {x!r} vs {y!r} (n = {n})")
    return bad


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_path():
    """evaluation_depth.py in the reference tree (oracle/ref_loader.py REF_ROOT; present on the authoring machine only)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return os.path.join(ref_loader.REF_ROOT, REF_EVAL)


def reference_eval_depth():
    """The reference's eval_depth, its module loaded from the reference tree with a stand-in for the Chamfer import (unused by it)."""
    import importlib.util
    path = reference_path()
    stub = types.ModuleType("unidepth.utils.chamfer_distance")

    class ChamferDistance:                      # eval_depth never calls it; the module builds one at import time
        def __call__(self, *a, **k):
            raise NotImplementedError

    stub.ChamferDistance = ChamferDistance
    saved = {k: sys.modules.get(k) for k in ("unidepth", "unidepth.utils", "unidepth.utils.chamfer_distance")}
    sys.modules.setdefault("unidepth", types.ModuleType("unidepth"))
    sys.modules.setdefault("unidepth.utils", types.ModuleType("unidepth.utils"))
    sys.modules["unidepth.utils.chamfer_distance"] = stub
    try:
        spec = importlib.util.spec_from_file_location("_ref_evaluation_depth_2d", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.eval_depth


def reference_outputs(ref_eval, name):
    gts, preds, masks, max_depth = case_inputs(name)
    with torch.no_grad():
        res = ref_eval(gts, preds, masks, max_depth=max_depth)
    return {k: v.numpy().astype(np.float32) for k, v in res.items()}, list(res)


def main():
    ref = reference_eval_depth()
    out = {}
    for name in CASES:
        vals, order = reference_outputs(ref, name)
        assert tuple(order) == KEYS, order
        for k, v in vals.items():
            out[f"{name}.{k}"] = v
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
