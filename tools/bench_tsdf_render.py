"""Times tsdf.tsdf_render (ud_tsdf_render, csrc/tsdf_render.hip) against tsdf.tsdf_render_composition, the torch loop over the samples of
the march, on the GPU box: B = 1 and 8 volumes of 128^3 and 256^3 voxels fused by tsdf_integrate from the scene of tools/bench_tsdf.py
(four Pinhole views with weights and colours), rendered at 518 x 518 and 480 x 640 from poses beside the integrated views.

    pinhole          Pinhole cameras
    mixed            images cycling through Pinhole, EUCM, Spherical and MEI (B = 1: MEI, the costliest unprojection)
    +nc              the same with normals and colours

The march runs from 0.5 to 4.0 in steps of a voxel (176 samples at 128^3, 351 at 256^3); the volume covers z = 1.22 .. 3.78.  Every
workload times the kernel's four forms -- a wave as 64 pixels of a row or as an 8 x 8 patch, the clip on or off -- and the composition.
Before timing, every output of the default form is compared with the composition's bit for bit at the timed size, and the four forms with
each other.  Time per call in a full queue of calls (events around each call, median of a window; three windows per arm after a warm-up,
the default form (rows, clipped) alternating with the composition on the same GPU in the same process); a window holds as many calls as fit a quarter
of a second, between 2 and 200.  The times are events around Python calls on cache-warm buffers: a CALL RATE.  Kernel times come from a run
of their own:
    rocprofv3 --kernel-trace -d DIR -o render -- python tools/bench_tsdf_render.py --kernels-only
which launches every form of every workload 5 times in the order of the table; --trace DIR/render_results.db (the profiler's SQLite
output) then adds the median duration of each group of 5 tr_render_kernel dispatches.
Prints one JSON line and writes the table to --out (default profiles/tsdf_render_bench.txt), one workload at a time.
    python tools/bench_tsdf_render.py [--out PATH] [--kernels-only] [--trace PATH] [--resources TEXT] [--grids 128,256] [--batches 1,8]"""
import argparse
import json
import math
import os
import sqlite3
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_tsdf as bt  # noqa: E402
from unidepth_amd import gtpoints, tsdf  # noqa: E402

WINDOWS, TRACE_CALLS = 3, 5
PINHOLE, EUCM, SPHERICAL, MEI = 1, 2, 3, 6
WORKLOADS = ("pinhole", "mixed", "pinhole+nc", "mixed+nc")
FORMS = (("rows clip", 0, 0), ("rows full", 0, 1), ("patch clip", 1, 0), ("patch full", 1, 1))      # name, wave_patch, full_scan
NEAR, FAR = 0.5, 4.0


def row(model, H, W):
    if model == SPHERICAL:
        hfov = math.radians(35.0)
        return [0.7 * W, 0.7 * W, W / 2, H / 2, W, H, hfov, math.atan(math.tan(hfov) * H / W)]
    return bt.CAMERAS[model](H, W)


def cameras(models, H, W):
    out = torch.zeros(len(models), 16)
    for b, m in enumerate(models):
        r = row(m, H, W)
        out[b, :len(r)] = torch.tensor(r)
    return gtpoints.PreparedCamera(out.cuda(), models)


def volume(N, B):
    """the colour volume of bench_tsdf's scene (V = 4 Pinhole views of 480 x 640 with weights and colours), B copies of it"""
    vol, _ = bt.workloads(N, 4, 480, 640)["pinhole+cw"][0]()
    rep = lambda t: t.repeat((B,) + (1,) * (t.ndim - 1)).contiguous()           # noqa: E731
    return tsdf.TsdfVolume(rep(vol.tsdf), rep(vol.weight), rep(vol.color), vol.origin, vol.voxel_size)


def poses(B):
    """volume to camera [B,3,4]: beside and between the integrated views, turned a little about y"""
    T = torch.zeros(B, 3, 4)
    for b in range(B):
        a = 0.08 * (b - (B - 1) / 2) / max(B - 1, 1) + 0.03
        R = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
        T[b, :, :3] = R
        T[b, :, 3] = -R @ torch.tensor([0.25 - 0.5 * b / max(B - 1, 1), 0.05, 0.0])
    return T.cuda()


def with_form(patch, full, fn):
    def run():
        saved = dict(tsdf._RENDER_OPTIONS)
        tsdf._RENDER_OPTIONS.update(wave_patch=patch, full_scan=full)
        try:
            return fn()
        finally:
            tsdf._RENDER_OPTIONS.update(saved)
    return run


def reps_for(fn):
    """how many calls fill a window of a quarter of a second, between 2 and 200, from one timed call after a warm-up"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return max(2, min(200, int(0.25 / max(time.perf_counter() - t0, 1e-6))))


def alternate(a, b):
    """one warm-up window of a (reps_for has warmed b), then WINDOWS windows of each, a b a b ...: ([ms of a], [ms of b], calls per window)"""
    ra, rb = reps_for(a), reps_for(b)
    bt.queue_ms(a, min(ra, 20))
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(bt.queue_ms(a, ra))
        tb.append(bt.queue_ms(b, rb))
    return ta, tb, ra, rb


def trace_medians(path, n_groups):
    db = sqlite3.connect(path)
    dur = [r[0] / 1e3 for r in db.execute("select duration from kernels where name like '%tr_render_kernel%' order by start")]
    assert len(dur) == TRACE_CALLS * n_groups, (len(dur), "dispatches in the trace")
    return [bt.median(dur[k:k + TRACE_CALLS]) for k in range(0, len(dur), TRACE_CALLS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_render_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch every form of every workload 5 times and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="render_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    ap.add_argument("--grids", default="128,256")
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_render.py needs a GPU"
    grids, batches = [int(x) for x in args.grids.split(",")], [int(x) for x in args.batches.split(",")]
    configs = [(N, B, tag, H, W) for N in grids for B in batches for tag, (H, W) in bt.SIZES.items()]
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace, len(configs) * len(WORKLOADS) * len(FORMS))
        except (OSError, sqlite3.Error, AssertionError) as e:
            print(f"bench_tsdf_render: kernel trace not used ({e!r})", file=sys.stderr)
    res = {"op": "tsdf_render (a TSDF volume ray-cast to depth, normals and colour, one launch)", "windows": WINDOWS}
    head = ["tools/bench_tsdf_render.py on " + torch.cuda.get_device_name(0) + ": ms per call (a call rate), median of a window of queued calls (n = calls "
            f"per window, as many as fit 0.25 s, 2 .. 200); {WINDOWS} windows per arm after a warm-up, tsdf_render (its default form: rows, clipped) "
            "alternating with tsdf_render_composition (torch, a loop over the samples); [..] = every window; ratio = fused / composition.",
            "forms: the four forms of the kernel, ms per call, each in windows of its own: patch / rows = a wave renders an 8 x 8 pixel patch / 64 "
            "pixels of a row; clip / full = samples outside the grid's box skipped / every sample visited.",
            "kernel = median tr_render_kernel duration (us) of 5 dispatches per form in a rocprofv3 --kernel-trace run of its own, in the order of "
            "the forms." if kernel_us else "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        head[-1:] = [args.resources, ""]
    if not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fh = open(args.out, "w")
        fh.write("\n".join(head) + "\n")
    k = 0
    vol, vol_key = None, None
    for N, B, tag, H, W in configs:
        if vol_key != (N, B):
            del vol
            torch.cuda.empty_cache()
            vol, vol_key = volume(N, B), (N, B)
        T = poses(B)
        key = f"n{N}_b{B}_{tag}"
        r = {}
        lines = [f"{key}  ({N}^3 voxels, B = {B} images of {H}x{W}, {int(math.floor((FAR - NEAR) / vol.voxel_size)) + 1} samples)"]
        for name in WORKLOADS:
            cyc = (PINHOLE,) if name.startswith("pinhole") else ((MEI,) if B == 1 else (PINHOLE, EUCM, SPHERICAL, MEI))
            cam = cameras(tuple(cyc[b % len(cyc)] for b in range(B)), H, W)
            kw = dict(near=NEAR, far=FAR, return_normals=name.endswith("+nc"), return_color=name.endswith("+nc"))
            call = lambda c=cam, kw=kw: tsdf.tsdf_render(vol, c, (H, W), T, **kw)                            # noqa: E731
            comp = lambda c=cam, kw=kw: tsdf.tsdf_render_composition(vol, c, (H, W), T, **kw)                # noqa: E731
            forms = [with_form(p, f, call) for _, p, f in FORMS]
            if args.kernels_only:
                for fn in forms:
                    for _ in range(TRACE_CALLS):
                        fn()
                torch.cuda.synchronize()
                continue
            outs = [fn() for fn in forms]
            want = comp()
            equal = all(bt.same_bits(a, b) for a, b in zip(outs[0], want)) and all(bt.same_bits(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
            share = float(outs[0][1].float().mean())
            del outs, want
            ta, tb, ra, rb = alternate(forms[0], comp)
            ma, mb = bt.median(ta), bt.median(tb)
            ft = [ma] + [bt.median([bt.queue_ms(fn, ra) for _ in range(WINDOWS)]) for fn in forms[1:]]
            r[name] = {"fused_ms": round(ma, 4), "fused_runs_ms": [round(t, 4) for t in ta], "fused_calls_per_window": ra, "composition_ms": round(mb, 3),
                       "composition_runs_ms": [round(t, 3) for t in tb], "composition_calls_per_window": rb, "ratio": round(ma / mb, 5),
                       "forms_ms": {f[0]: round(t, 4) for f, t in zip(FORMS, ft)}, "bit_equal": equal, "valid_share": round(share, 3)}
            ktxt = ""
            if kernel_us:
                ku = kernel_us[k:k + len(FORMS)]
                r[name]["kernel_us"] = {f[0]: round(t, 1) for f, t in zip(FORMS, ku)}
                ktxt = "  kernel " + " / ".join(f"{t:.1f}" for t in ku) + " us"
            k += len(FORMS)
            lines.append(f"  {name:11s} fused {ma:.4f} {[round(t, 4) for t in ta]} n={ra}  composition {mb:.2f} {[round(t, 2) for t in tb]} n={rb}  "
                         f"ratio {ma / mb:.5f}  forms " + " / ".join(f"{f[0]} {t:.4f}" for f, t in zip(FORMS, ft)) + f"{ktxt}  bit-equal {equal}  valid {share:.2f}")
        if args.kernels_only:
            continue
        res[key] = r
        fh.write("\n".join(lines) + "\n\n")
        fh.flush()
        print("\n".join(lines), file=sys.stderr, flush=True)
    if args.kernels_only:
        return
    fh.close()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
