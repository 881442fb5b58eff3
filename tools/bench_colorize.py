"""Times visualization.colorize_batch / demo_panel (ud_colorize, csrc/colorize.hip) next to (i) the torch composition of the same
arithmetic a user writes without it (normalise, scale, clamp, index a LUT, mask) and (ii) the reference's route, a device-to-host copy of
the maps and the host colorize once per image, on the same GPU, same process.  B = 8 at 518 x 518 and at 480 x 640:
  (a) one map with given limits   (b) one map auto-ranged (per-image min / max)   (c) the 2 x 2 demo panel rgb | gt / pred | error.
ud_colorize and the torch composition alternate; a sample is a window of CALLS back-to-back calls through the Python surface between two
device events, the figure the median of REPS samples after warm-up, per call.  That is the rate at which calls complete in a full queue:
the larger of the kernels' time and the host's time to submit a call, on buffers that are reread every call and fit the 256 MB
Infinity Cache.  It is NOT a kernel time and says nothing about HBM: "call_rate_GBps" is the algorithm's bytes (every source element
read once per pass, twice when auto-ranged, three bytes written per pixel) over that per-call time, named for what it is.  The host
route is a wall clock around copy + numpy (it ends synchronised), median of 5.  ud_colorize is compared byte for byte with the host
route before anything is timed; pixels where the torch composition differs are counted and reported.  Prints one JSON line.

    python tools/bench_colorize.py
    python tools/bench_colorize.py --only b8_518x518_given --calls 200     that case's ud_colorize calls alone and nothing timed: the
                                                                            program to put after `rocprofv3 --kernel-trace --stats --`
                                                                            for the kernels' own time (a run of its own)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import _lib, visualization  # noqa: E402

REPS, CALLS, WARM = 11, 1000, 3        # a window of 1000 calls is 14-350 ms: long against the clock's and the scheduler's grain


def inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = (3.0 + 2.5 * torch.sin(yy / 40.0) * torch.cos(xx / 55.0)).repeat(B, 1, 1) * (1.0 + 0.1 * torch.arange(B).view(B, 1, 1))
    pred = (gt * (0.9 + 0.2 * torch.rand(B, H, W, generator=g))).float()
    gt = torch.where(torch.rand(B, H, W, generator=g) < 0.1, torch.zeros(()), gt).float()          # pixels without ground truth
    rgb = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    return rgb.cuda(), pred.cuda(), gt.cuda()


def torch_colorize(v, lut, vmin, vmax):
    """The composition of the same arithmetic in torch: every operation its own kernel, each rounded to fp32 like ud_colorize."""
    if vmin is not None and vmax is not None:
        lo, den = np.float32(vmin).item(), np.float32(float(vmax) - float(vmin)).item()
    else:
        lo = v.amin(dim=(1, 2), keepdim=True) if vmin is None else torch.full((), vmin, device=v.device)
        hi = v.amax(dim=(1, 2), keepdim=True) if vmax is None else torch.full((), vmax, device=v.device)
        den = hi - lo
    x = (v - lo) / den * 256.0
    img = lut[x.clamp(0.0, 255.0).nan_to_num(0.0).long()]
    return torch.where(((x != x) | (v < 1e-4)).unsqueeze(-1), torch.zeros((), dtype=torch.uint8, device=v.device), img)


def torch_panel(rgb, pred, gt, lut_d, lut_e):
    e = torch.where(gt == 0, torch.zeros((), device=gt.device), (gt - pred).abs() / gt)
    top = torch.cat([rgb.permute(0, 2, 3, 1), torch_colorize(gt, lut_d, 0.01, 10.0)], dim=2)
    bot = torch.cat([torch_colorize(pred, lut_d, 0.01, 10.0), torch_colorize(e, lut_e, 0.0, 0.2)], dim=2)
    return torch.cat([top, bot], dim=1)


def host_route(maps, vmin, vmax, cmap):
    """The reference's route: the maps to the host, colorize per image in numpy."""
    h = maps.cpu().numpy()
    return np.stack([visualization.colorize(h[b], vmin, vmax, cmap) for b in range(h.shape[0])])


def host_panel(rgb, pred, gt):
    """demo.py's artifact the reference's way: everything to the host, three colorize calls and image_grid per image."""
    r, p, g = rgb.cpu().numpy(), pred.cpu().numpy(), gt.cpu().numpy()
    out = []
    for i in range(r.shape[0]):
        with np.errstate(all="ignore"):
            e = np.abs(g[i] - p[i]) / g[i]
        e[g[i] == 0.0] = 0.0
        out.append(visualization.image_grid([r[i].transpose(1, 2, 0), visualization.colorize(g[i], 0.01, 10.0, "magma_r"),
                                             visualization.colorize(p[i], 0.01, 10.0, "magma_r"), visualization.colorize(e, 0.0, 0.2, "coolwarm")], 2, 2))
    return np.stack(out)


def alternate_ms(fa, fb):
    for _ in range(WARM):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        for fn, t in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / CALLS)
    return sorted(ta)[REPS // 2], sorted(tb)[REPS // 2]


def host_ms(fn, reps=5):
    fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="run this case's ud_colorize calls alone, untimed (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=200, help="calls of the --only case")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_colorize needs the GPU"
    res = {"op": "ud_colorize (u8 HWC out)", "reps": REPS, "calls_per_sample": CALLS}
    lut_d, lut_e = visualization._lut("magma_r", torch.device("cuda", 0)), visualization._lut("coolwarm", torch.device("cuda", 0))
    for B, H, W in ((8, 518, 518), (8, 480, 640)):
        rgb, pred, gt = inputs(B, H, W)
        npx = B * H * W
        work = torch.empty(int(_lib.lib.ud_colorize_work_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
        out1 = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
        cases = {
            "given": (lambda: visualization.colorize_batch(pred, 0.01, 10.0, out=out1), lambda: torch_colorize(pred, lut_d, 0.01, 10.0),
                      lambda: host_route(pred, 0.01, 10.0, "magma_r"), 1, npx * (4 + 3)),
            "auto": (lambda: visualization.colorize_batch(pred, None, None, out=out1, workspace=work), lambda: torch_colorize(pred, lut_d, None, None),
                     lambda: host_route(pred, None, None, "magma_r"), 2, npx * (4 + 4 + 3)),
            "panel2x2": (lambda: visualization.demo_panel(rgb, pred, gt), lambda: torch_panel(rgb, pred, gt, lut_d, lut_e),
                         lambda: host_panel(rgb, pred, gt), 1, npx * (3 + 4 + 4 + 8 + 12)),
        }
        for name, (ours, theirs, host, launches, nbytes) in cases.items():
            if args.only:
                if args.only == f"b{B}_{H}x{W}_{name}":
                    for _ in range(args.calls):
                        ours()
                    torch.cuda.synchronize()
                    print(json.dumps({"only": args.only, "calls": args.calls, "launches_per_call": launches, "MB_per_call": round(nbytes / 1e6, 1)}))
                    return
                continue
            a, b = ours(), theirs()
            assert np.array_equal(a.cpu().numpy(), host()), name                 # the reference's route, byte for byte
            differs = int((a != b).any(dim=-1).sum())                            # torch's own division / rounding may differ: reported
            ms, ms_torch = alternate_ms(ours, theirs)
            rec = {"launches": launches, "ud_colorize_ms": round(ms, 4), "torch_compose_ms": round(ms_torch, 4), "speedup": round(ms_torch / ms, 2),
                   "MB_per_call": round(nbytes / 1e6, 1), "call_rate_GBps": round(nbytes / ms / 1e6, 1)}
            rec["torch_compose_differing_px"] = differs
            rec["d2h_plus_host_colorize_ms"] = round(host_ms(host), 2)
            res[f"b{B}_{H}x{W}_{name}"] = rec
    assert not args.only, f"unknown case {args.only}"
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
