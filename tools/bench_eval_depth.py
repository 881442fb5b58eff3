"""Times eval_ops.eval_depth (ud_eval_depth, csrc/evaldepth.hip) on the GPU box, next to a torch restatement of the reference's
per-image loop (boolean-mask indexing, one small op chain per metric, 100 threshold means for d_auc, torch.median) on the same GPU and
inputs.  Two cases: B = 8 at 480 x 640 (dense mask, pred at full size) and B = 8 at 375 x 1242 (~10 % mask, pred 266 x 882).
Prints one JSON line.   python tools/bench_eval_depth.py"""
import importlib.util
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import eval_ops  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_eval_depth", os.path.join(ROOT, "tools", "make_golden_eval_depth.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)


def gpu_ms(fn, reps=9):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))[reps // 2]


def wall_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[reps // 2]


def torch_loop(gts, preds, masks, max_depth=None):
    """The reference's scoring loop restated in plain torch ops (what a user runs without the engine)."""
    def ratio(g, p):
        return torch.maximum(g / p, p / g)

    def med_scale(g, p):
        return p * torch.median(g) / torch.median(p)

    def lsq(g, p):
        A = torch.stack([p, torch.ones_like(p)], dim=1)
        st = torch.inverse(A.T @ A + 1e-9 * torch.eye(2, device=p.device)) @ (A.T @ g.unsqueeze(1))
        s, t = st.squeeze().chunk(2, dim=0)
        return p * s + t

    def frac_below(g, p, th):
        return (ratio(g, p) < th).float().mean()

    def dauc(g, p):
        e = torch.linspace(0.01, 5.0, steps=100, device=g.device)
        fr = [frac_below(g, p, 1.25 ** x) for x in e]
        return torch.trapz(torch.tensor(fr, device=g.device), e) / 5.0

    fns = {"d1": lambda g, p: frac_below(g, p, 1.25), "d2": lambda g, p: frac_below(g, p, 1.25 ** 2),
           "d3": lambda g, p: frac_below(g, p, 1.25 ** 3), "rmse": lambda g, p: ((g - p) ** 2).mean().sqrt(),
           "rmselog": lambda g, p: ((g.log() - p.log()) ** 2).mean().sqrt(), "arel": lambda g, p: ((g - p).abs() / g).mean(),
           "sqrel": lambda g, p: ((g - p) ** 2 / g).mean(), "log10": lambda g, p: (p.log10() - g.log10()).abs().mean(),
           "silog": lambda g, p: 100 * torch.std(p.log() - g.log()), "medianlog": lambda g, p: 100 * (p.log() - g.log()).median().abs(),
           "d_auc": dauc, "tau": lambda g, p: frac_below(g, p, 1.03)}
    out = {}
    preds = F.interpolate(preds, gts.shape[-2:], mode="bilinear")
    for gt, pred, mask in zip(gts, preds, masks):
        if max_depth is not None:
            mask = mask & (gt <= max_depth)
        g, p = gt[mask], pred[mask]
        for name, fn in fns.items():
            if name in ("d1", "arel", "tau"):
                out.setdefault(f"{name}_ssi", []).append(fn(g, lsq(g, p)))
                out.setdefault(f"{name}_si", []).append(fn(g, med_scale(g, p)))
            out.setdefault(name, []).append(fn(g, p))
    return {k: torch.stack(v) for k, v in out.items()}


def main():
    res = {"op": "eval_depth (18 metrics per image)"}
    cases = {"b8_480x640_dense": (8, (480, 640), (480, 640), "dense"), "b8_375x1242_sparse_resampled": (8, (375, 1242), (266, 882), "sparse")}
    for tag, (B, HW, hw, kind) in cases.items():
        gts, preds, masks = mg.random_inputs(torch.Generator().manual_seed(0), B, HW, hw, kind)
        if kind == "dense":
            masks[:] = True
        gts, preds, masks = gts.cuda(), preds.cuda(), masks.cuda()
        ms = gpu_ms(lambda: eval_ops.eval_depth(gts, preds, masks))
        loop = wall_ms(lambda: torch_loop(gts, preds, masks))
        nbytes = B * HW[0] * HW[1] * 5 + B * hw[0] * hw[1] * 4            # gt + mask + pred, once
        res[tag] = {"eval_depth_ms": round(ms, 4), "torch_loop_ms": round(loop, 2), "speedup": round(loop / ms, 1),
                    "passes": 5, "launches": 11, "GBps_per_pass_equiv": round(5 * nbytes / ms / 1e6, 1)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
