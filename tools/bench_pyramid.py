"""Times pyramid.depth_pyramid (ud_depth_pyramid, csrc/pyramid.hip) against pyramid.depth_pyramid_composition, and
pyramid.track_camera_pyramid against icp.track_camera, on the GPU box: B = 1 and 8 at 518 x 518 and 480 x 640.

    pyramid     depth_pyramid(levels=3) with r = 0 / 2 / 4, with and without weights, both tile shapes (32 x 32 and 64 x 16), each
                alternating with the composition: time per call in a full queue of calls (events around each call, median of a window;
                three windows per arm after a warm-up, tools/bench_icp.py's scheme).  A CALL RATE, close to the host's submission rate
                where the kernel is short.
    track       track_camera_pyramid(iters=(10, 5, 4)) against track_camera(iters=10) and track_camera(iters=19) on tools/bench_icp.py's
                smooth scene (a Pinhole frame against Pinhole model maps, the start 1.8 degrees / 0.054 from the truth, dist_tol 0.1; the
                model maps of level l are the analytic surface through pyramid_cameras(...)[l]), with the final pose error of each (the
                truth is the identity: rotation angle in degrees, length of the translation), and against its own composition
                (depth_pyramid_composition, then track_camera_composition level by level).

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace -d DIR -o pyr -- python tools/bench_pyramid.py --kernels-only
which runs, per pyramid workload in the order of the table, depth_pyramid 50 times with each tile shape; --trace DIR/.../pyr_results.db
then adds the median duration of each group's 50 py_kernel dispatches and the algorithmic bytes per second: depth (and weights) read once,
every level written once -- B * H * W * 4 * (1 + 21/16) bytes, twice that with weights.
Prints one JSON line and writes the table to --out (default profiles/pyramid_bench.txt).
    python tools/bench_pyramid.py [--out PATH] [--kernels-only] [--trace PATH] [--note TEXT]"""
import argparse
import json
import math
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_icp as bi  # noqa: E402
from unidepth_amd import icp, pyramid  # noqa: E402

REPS, REPS_COMP, REPS_TRACK, REPS_TRACK_COMP, WINDOWS, TRACE_CALLS = 200, 10, 20, 2, 3, 50
RADII, LEVELS, TILES = (0, 2, 4), 3, (1, 2)
ITERS = (10, 5, 4)
SIGMA_SPACE, SIGMA_RANGE, GATE = 1.5, 0.02, 0.05


def alternate(arms):
    """arms: [(fn, reps)]; one warm-up window of each, then WINDOWS rounds over the arms in turn -> [[ms per window] per arm]"""
    for fn, reps in arms:
        bi.queue_ms(fn, max(reps // 10, 2))
    out = [[] for _ in arms]
    for _ in range(WINDOWS):
        for k, (fn, reps) in enumerate(arms):
            out[k].append(bi.queue_ms(fn, reps))
    return out


def frame(B, H, W):
    """bench_icp's surface through a Pinhole with noise of 1 % and holes: the depth and a confidence map in 0.5 .. 2"""
    cam = bi.camera(bi.PINHOLE, B, H, W)
    g = torch.Generator(device="cuda").manual_seed(5)
    d = bi.surface(cam, B, H, W)[0]
    d = d * (1 + 0.01 * torch.randn(d.shape, device="cuda", generator=g))
    d = torch.where(torch.rand(d.shape, device="cuda", generator=g) < 0.02, torch.zeros_like(d), d)
    w = 0.5 + 1.5 * torch.rand(d.shape, device="cuda", generator=g)
    return d.contiguous(), w.contiguous()


def with_tile(tile, fn):
    def run():
        pyramid._LAUNCH_OPTIONS["tile"] = tile
        try:
            return fn()
        finally:
            pyramid._LAUNCH_OPTIONS["tile"] = 0
    return run


def pyramid_workloads(B, H, W):
    d, w = frame(B, H, W)
    for r in RADII:
        f = pyramid.prepare_depth_filter(r, SIGMA_SPACE, SIGMA_RANGE, "cuda") if r else None
        for use_w in (False, True):
            kw = dict(filter=f, gate=GATE, weights=w if use_w else None)
            yield f"r{r}_{'w' if use_w else 'nw'}", use_w, (lambda kw=kw: pyramid.depth_pyramid(d, LEVELS, **kw)), (lambda kw=kw: pyramid.depth_pyramid_composition(d, LEVELS, **kw))


def flat(res):
    return list(res[0]) + list(res[1]) if isinstance(res, tuple) else list(res)


def pose_error(T):
    R, t = T[0, :, :3].double().cpu(), T[0, :, 3].double().cpu()
    s = 0.5 * torch.tensor([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return math.degrees(math.atan2(float(s.norm()), float((R.trace() - 1) / 2))), float(t.norm())


def track_workload(B, H, W):
    """bench_icp's pin_pin scene with the model maps of every level"""
    model = bi.camera(bi.PINHOLE, B, H, W)
    cams = pyramid.pyramid_cameras(model, B, LEVELS, "cuda")
    levels = []
    for l, c in enumerate(cams):
        h, w = H >> l, W >> l
        _, mp, mn = bi.surface(c, B, h, w)
        mv = torch.zeros(B, 1, h, w, dtype=torch.bool, device="cuda")
        mv[:, :, 1:-1, 1:-1] = True
        levels.append((mp, mn, mv, c))
    depth = bi.surface(model, B, H, W)[0]
    return depth, cams, levels, bi.start(B)


def track_composition(depth, cams, levels, T):
    dl = pyramid.depth_pyramid_composition(depth, LEVELS)
    for l in reversed(range(LEVELS)):
        T, _ = icp.track_camera_composition(dl[l], cams[l], *levels[l], T, iters=ITERS[l], dist_tol=bi.DIST_TOL)
    return T


def trace_medians(path, n_groups):
    db = sqlite3.connect(path)
    dur = [r[0] / 1e3 for r in db.execute("select duration from kernels where name like '%py_kernel%' and name not like '%copy_kernel%' order by start")]   # torch's copy_kernel shares the letters
    assert len(dur) == TRACE_CALLS * n_groups, (len(dur), "dispatches of py_kernel in the trace, expected", TRACE_CALLS * n_groups)
    return [bi.median(dur[k:k + TRACE_CALLS]) for k in range(0, len(dur), TRACE_CALLS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="run depth_pyramid 50 times per workload and tile and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="pyr_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--note", default="", help="a line copied into the table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pyramid.py needs a GPU"
    n_groups = len(bi.configs()) * len(RADII) * 2 * len(TILES)
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace, n_groups)
        except (OSError, sqlite3.Error, AssertionError) as e:
            print(f"bench_pyramid: kernel trace not used ({e!r})", file=sys.stderr)
    rd = lambda ts: [round(t, 4) for t in ts]                            # noqa: E731
    res = {"op": "depth_pyramid (one launch) and track_camera_pyramid", "reps": REPS, "reps_composition": REPS_COMP, "windows": WINDOWS}
    lines = ["tools/bench_pyramid.py on " + torch.cuda.get_device_name(0) + f": ms per call (a call rate), median of a window of queued calls ({REPS} fused, "
             f"{REPS_COMP} of the composition; track: {REPS_TRACK} and {REPS_TRACK_COMP}); {WINDOWS} windows per arm after a warm-up, the arms alternating;",
             "[..] = every window; ratio = fused (default tile) / composition.  levels = 3; rN = filter radius N; w / nw = with / without weights.",
             "kernel = median py_kernel duration of 50 dispatches in a rocprofv3 --kernel-trace run of its own, per tile shape; GB/s = the algorithmic "
             "bytes (inputs read once, every level written once) over that time." if kernel_us else "kernel times: not measured in this run (no --trace).", ""]
    if args.note:
        lines[-1:] = [args.note, ""]
    k = 0
    slower = []
    for tag, H, W, B in bi.configs():
        key = f"b{B}_{tag}"
        r = {}
        lines.append(f"{key}  (B = {B}, {H * W} pixels per image)")
        for name, use_w, fused, comp in pyramid_workloads(B, H, W):
            if args.kernels_only:
                for tile in TILES:
                    run = with_tile(tile, fused)
                    for _ in range(TRACE_CALLS):
                        run()
                torch.cuda.synchronize()
                continue
            equal = all(bi.same_bits(x, y) for t in TILES for x, y in zip(flat(with_tile(t, fused)()), flat(comp())))
            t32, t64, tc = alternate([(with_tile(1, fused), REPS), (with_tile(2, fused), REPS), (comp, REPS_COMP)])
            m32, m64, mc = bi.median(t32), bi.median(t64), bi.median(tc)
            r[name] = {"tile32x32_ms": round(m32, 4), "tile32x32_runs_ms": rd(t32), "tile64x16_ms": round(m64, 4), "tile64x16_runs_ms": rd(t64),
                       "composition_ms": round(mc, 4), "composition_runs_ms": rd(tc), "ratio": round(m32 / mc, 4), "bit_equal": equal}
            if m32 > mc:
                slower.append(f"{key} {name}")
            ktxt = ""
            if kernel_us:
                us = kernel_us[k:k + len(TILES)]
                nbytes = B * H * W * 4 * (1 + 21 / 16) * (2 if use_w else 1)
                r[name].update(kernel_us={"32x32": round(us[0], 1), "64x16": round(us[1], 1)}, algorithmic_GBps=round(nbytes / (us[0] * 1e-6) / 1e9, 1))
                ktxt = f"  kernel 32x32 {us[0]:.1f} us ({nbytes / (us[0] * 1e-6) / 1e9:.0f} GB/s), 64x16 {us[1]:.1f} us"
            k += len(TILES)
            lines.append(f"  {name:6s} 32x32 {m32:.4f} {rd(t32)}  64x16 {m64:.4f} {rd(t64)}  composition {mc:.3f} {rd(tc)}  ratio {m32 / mc:.4f}  bit-equal {equal}{ktxt}")
        if not args.kernels_only:
            depth, cams, levels, T0 = track_workload(B, H, W)
            a0 = (depth, cams[0], *levels[0], T0)
            pyr = lambda: pyramid.track_camera_pyramid(depth, cams, levels, T0, iters=ITERS, dist_tol=bi.DIST_TOL)          # noqa: E731
            t10 = lambda: icp.track_camera(*a0, iters=10, dist_tol=bi.DIST_TOL)                                             # noqa: E731
            t19 = lambda: icp.track_camera(*a0, iters=19, dist_tol=bi.DIST_TOL)                                             # noqa: E731
            comp = lambda: track_composition(depth, cams, levels, T0)                                                       # noqa: E731
            errs = {n: pose_error(f()[0]) for n, f in (("pyramid", pyr), ("track10", t10), ("track19", t19))}
            tp, ta, tb, tcmp = alternate([(pyr, REPS_TRACK), (t10, REPS_TRACK), (t19, REPS_TRACK), (comp, REPS_TRACK_COMP)])
            mp_, ma, mb, mcmp = bi.median(tp), bi.median(ta), bi.median(tb), bi.median(tcmp)
            r["track"] = {"pyramid_10_5_4_ms": round(mp_, 4), "pyramid_runs_ms": rd(tp), "track10_ms": round(ma, 4), "track10_runs_ms": rd(ta),
                          "track19_ms": round(mb, 4), "track19_runs_ms": rd(tb), "pyramid_composition_ms": round(mcmp, 3), "pose_error_deg_len": errs}
            if mp_ > mcmp:
                slower.append(f"{key} track")
            lines.append(f"  track  pyramid (10, 5, 4) {mp_:.4f} {rd(tp)}  track_camera(iters=10) {ma:.4f} {rd(ta)}  track_camera(iters=19) {mb:.4f} {rd(tb)}  "
                         f"its composition {mcmp:.2f} {rd(tcmp)}")
            lines.append("         final pose error (degrees, translation): " + ", ".join(f"{n} {e[0]:.2e} / {e[1]:.2e}" for n, e in errs.items()))
        res[key] = r
        lines.append("")
    if args.kernels_only:
        return
    lines.append("slower than its composition: " + (", ".join(slower) if slower else "none"))
    res["slower_than_composition"] = slower
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
