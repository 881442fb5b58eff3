"""Times tsdf.tsdf_integrate (ud_tsdf_integrate, csrc/tsdf.hip) against the composition it fuses -- tsdf.tsdf_integrate_composition: per
view project_camera, remap(mode="nearest") and the element-wise update -- and tsdf.tsdf_points (ud_tsdf_points) against a torch
composition of the same definition (comparisons, nonzero, indexing, a sort into slot order), on the GPU box: B = 1, grids of 128^3 and
256^3 voxels, V = 4 and 8 views of 518 x 518 and 480 x 640, into a fresh volume.

    pinhole          Pinhole views
    mixed            views cycling through Pinhole, EUCM, Fisheye624 and MEI
    +cw              the same with src_weights and images (a colour volume)

The scene is the plane z = 2.5 with a block at 2.1, seen by views translated sideways, a twentieth of every view's pixels empty; the grid is
a cube of side 2.56 around the plane.  Before timing, every output of the fused call (tsdf, weight, colour, count) is compared with the
composition's bit for bit at the timed size, and so are the points.  Time per call in a full queue of calls (events around each call,
median of a window; three windows per arm after a warm-up, the two arms alternating on the same GPU in the same process); a window holds as
many calls as fit a quarter of a second, between 5 and 200, so the composition's windows hold fewer calls than the fused call's.  The times
are events around Python calls on cache-warm buffers: a CALL RATE.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace -d DIR -o tsdf -- python tools/bench_tsdf.py --kernels-only
which launches every fused integration 20 times in the order of the table; --trace DIR/tsdf_results.db (the profiler's SQLite output) then
adds the median duration of each workload's 20 ts_integrate_kernel dispatches and the algorithmic bytes per second: the volume's state
written once (a fresh volume is not read), every view read at most once.
Prints one JSON line and writes the table to --out (default profiles/tsdf_bench.txt).
    python tools/bench_tsdf.py [--out PATH] [--kernels-only] [--trace PATH] [--resources TEXT] [--grids 128,256]"""
import argparse
import json
import os
import sqlite3
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import gtpoints, pointcloud, tsdf  # noqa: E402

WINDOWS, TRACE_CALLS, WINDOW_S = 3, 20, 0.25
PINHOLE, EUCM, FISHEYE624, MEI = 1, 2, 5, 6
SIZES = {"518x518": (518, 518), "480x640": (480, 640)}
VIEWS = (4, 8)
WORKLOADS = ("pinhole", "mixed", "pinhole+cw", "mixed+cw")
SIDE, PLANE, BLOCK = 2.56, 2.5, 2.1


def queue_ms(fn, reps):
    """median time per call with `reps` calls enqueued back to back"""
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))[reps // 2]


def reps_for(fn):
    """how many calls fill a window of WINDOW_S seconds, between 5 and 200, from one timed call after a warm-up"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return max(5, min(200, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))


def alternate(a, b):
    """one warm-up window of each, then WINDOWS windows of each, a b a b ...: ([ms of a], [ms of b], calls per window of a, of b)"""
    ra, rb = reps_for(a), reps_for(b)
    queue_ms(a, min(ra, 20))
    queue_ms(b, min(rb, 20))
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(queue_ms(a, ra))
        tb.append(queue_ms(b, rb))
    return ta, tb, ra, rb


def median(ts):
    return sorted(ts)[len(ts) // 2]


# a view of about +-35 degrees horizontally for every model
CAMERAS = {
    PINHOLE: lambda H, W: [0.7 * W, 0.7 * W + 1, W / 2 + 1, H / 2 - 1],
    EUCM: lambda H, W: [0.66 * W, 0.66 * W + 1, W / 2 - 1, H / 2 + 1, 0.55, 1.05],
    FISHEYE624: lambda H, W: [0.8 * W, 0.8 * W + 1, W / 2, H / 2, -0.02, 0.004, -0.001, 2e-4, -1e-4, 1e-5, 1e-3, -1e-3, 2e-3, 1e-4, -1e-3, 2e-4],
    MEI: lambda H, W: [1.3 * W, 1.3 * W + 1, W / 2, H / 2 + 1, -0.1, 0.02, 1e-3, -1e-3, 0.9],
}


def camera(model, H, W):
    out = torch.zeros(1, 16)
    r = CAMERAS[model](H, W)
    out[:, :len(r)] = torch.tensor(r)
    return gtpoints.PreparedCamera(out.cuda(), (model,))


def workloads(N, V, H, W):
    """name -> (fused call, composition call), both returning (TsdfVolume, count) of a fresh volume of N^3 voxels"""
    g = torch.Generator().manual_seed(0)
    T = torch.eye(4)[:3].repeat(V, 1, 1)
    T[:, 0, 3] = torch.linspace(-0.4, 0.4, V)
    T = T.cuda()
    depths = torch.full((1, V, H, W), PLANE)
    depths[:, :, H // 3:2 * H // 3, W // 3:W // 2] = BLOCK
    depths[torch.rand(1, V, H, W, generator=g) < 0.05] = 0.0
    depths = depths.cuda()
    weights = (0.5 + torch.rand(1, V, H, W, generator=g)).cuda()
    images = torch.randint(0, 256, (1, V, 3, H, W), generator=g, dtype=torch.uint8).cuda()
    vs = SIDE / N
    kw = dict(grid_shape=(N, N, N), origin=torch.tensor([[-SIDE / 2, -SIDE / 2, PLANE - SIDE / 2]], device="cuda"), voxel_size=vs, trunc=4 * vs,
              return_count=True)
    out = {}
    for name in WORKLOADS:
        models = (PINHOLE,) if name.startswith("pinhole") else (PINHOLE, EUCM, FISHEYE624, MEI)
        cams = [camera(models[v % len(models)], H, W) for v in range(V)]
        k = dict(kw, src_weights=weights, images=images) if name.endswith("+cw") else kw
        out[name] = ((lambda c=cams, k=k: tsdf.tsdf_integrate(None, depths, c, T, **k)),
                     (lambda c=cams, k=k: tsdf.tsdf_integrate_composition(None, depths, c, T, **k)))
    return out


def points_composition(vol, min_weight=1.0):
    """tsdf_points' definition in torch for B = 1: per axis the comparisons on shifted views, nonzero, indexing and the payload; the rows
    of the three axes sorted into slot order -> PointCloud"""
    t, w, o, vs = vol.tsdf[0], vol.weight[0], vol.origin[0], vol.voxel_size
    Nz, Ny, Nx = t.shape
    slots, xyzs, rgbs = [], [], []
    for axis, dim in ((0, 2), (1, 1), (2, 0)):
        n = t.shape[dim]
        a, b = t.narrow(dim, 0, n - 1), t.narrow(dim, 1, n - 1)
        ok = (w.narrow(dim, 0, n - 1) >= min_weight) & (w.narrow(dim, 1, n - 1) >= min_weight) & ~a.isnan() & ~b.isnan() & ((a < 0) != (b < 0))
        iz, iy, ix = ok.nonzero().unbind(1)
        a, b = a[iz, iy, ix], b[iz, iy, ix]
        tt = a / (a - b)
        c = [o[k] + (i.float() + 0.5) * vs for k, i in enumerate((ix, iy, iz))]
        c[axis] = c[axis] + tt * vs
        xyzs.append(torch.stack(c, dim=1))
        slots.append(((iz * Ny + iy) * Nx + ix) * 3 + axis)
        if vol.color is not None:
            step = [0, 0, 0]
            step[dim] = 1
            c0, c1 = vol.color[0][:, iz, iy, ix], vol.color[0][:, iz + step[0], iy + step[1], ix + step[2]]
            rgbs.append((c0 + tt * (c1 - c0)).round().clamp(0, 255).to(torch.uint8).t())
    order = torch.cat(slots).argsort()
    xyz = torch.cat(xyzs)[order]
    total = torch.tensor([xyz.shape[0]], device=xyz.device)
    return pointcloud.PointCloud(xyz, torch.cat(rgbs)[order] if rgbs else None, None, total, torch.cat([torch.zeros_like(total), total]))


def same_bits(a, b):
    if a is None or b is None:
        return a is b
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def configs(grids):
    return [(N, tag, H, W, V) for N in grids for tag, (H, W) in SIZES.items() for V in VIEWS]


def view_bytes(name, V, H, W):
    return V * H * W * (4 + (4 + 3 if name.endswith("+cw") else 0))


def volume_bytes(name, N):
    return N ** 3 * (4 + 4 + 1 + (12 if name.endswith("+cw") else 0))


def trace_medians(path, n_groups):
    """the kernel trace of a --kernels-only run: the median duration (us) of each consecutive group of TRACE_CALLS ts_integrate_kernel dispatches"""
    db = sqlite3.connect(path)
    dur = [r[0] / 1e3 for r in db.execute("select duration from kernels where name like '%ts_integrate_kernel%' order by start")]
    assert len(dur) == TRACE_CALLS * n_groups, (len(dur), "dispatches in the trace")
    return [median(dur[k:k + TRACE_CALLS]) for k in range(0, len(dur), TRACE_CALLS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch every fused integration 20 times and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="tsdf_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    ap.add_argument("--grids", default="128,256", help="the grid sides to run, comma separated")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf.py needs a GPU"
    grids = [int(x) for x in args.grids.split(",")]
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace, len(configs(grids)) * len(WORKLOADS))
        except (OSError, sqlite3.Error, AssertionError) as e:           # the call times do not depend on the trace
            print(f"bench_tsdf: kernel trace not used ({e!r})", file=sys.stderr)
    res = {"op": "tsdf_integrate (depth views fused into a TSDF volume, one launch) and tsdf_points", "windows": WINDOWS, "window_s": WINDOW_S}
    lines = ["tools/bench_tsdf.py on " + torch.cuda.get_device_name(0) + ": ms per call (a call rate), median of a window of queued calls (n = calls per "
             f"window, as many as fit {WINDOW_S} s, 5 .. 200); {WINDOWS} windows per arm after a warm-up, the fused call alternating with its composition:",
             "tsdf_integrate with tsdf_integrate_composition (per view: project_camera, remap nearest and the element-wise update), tsdf_points with a "
             "torch composition (nonzero / indexing / sort); B = 1, a fresh volume; [..] = every window; ratio = fused / composition.",
             "kernel = median ts_integrate_kernel duration of 20 dispatches in a rocprofv3 --kernel-trace run of its own; GB/s = the algorithmic bytes "
             "(tsdf + weight + count, + colour, written once; every view's depth, + weight + colour, read once) over that time." if kernel_us
             else "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        lines[-1:] = [args.resources, ""]
    k = 0
    for N, tag, H, W, V in configs(grids):
        key = f"n{N}_v{V}_{tag}"
        r = {}
        lines.append(f"{key}  ({N}^3 voxels, V = {V} views of {H}x{W})")
        for name, (fused, comp) in workloads(N, V, H, W).items():
            if args.kernels_only:
                for _ in range(TRACE_CALLS):
                    fused()
                torch.cuda.synchronize()
                continue
            (vol, count), (cvol, ccount) = fused(), comp()
            equal = all(same_bits(a, b) for a, b in ((vol.tsdf, cvol.tsdf), (vol.weight, cvol.weight), (vol.color, cvol.color), (count, ccount)))
            share = float((count > 0).float().mean())
            del cvol, ccount
            ta, tb, ra, rb = alternate(fused, comp)
            ma, mb = median(ta), median(tb)
            r[name] = {"fused_ms": round(ma, 4), "fused_runs_ms": [round(t, 4) for t in ta], "fused_calls_per_window": ra, "composition_ms": round(mb, 4),
                       "composition_runs_ms": [round(t, 4) for t in tb], "composition_calls_per_window": rb, "ratio": round(ma / mb, 4),
                       "bit_equal": equal, "updated_share": round(share, 3)}
            ktxt = ""
            if kernel_us:
                gbs = (volume_bytes(name, N) + view_bytes(name, V, H, W)) / (kernel_us[k] * 1e-6) / 1e9
                r[name]["kernel_us"], r[name]["algorithmic_GBps"] = round(kernel_us[k], 1), round(gbs, 1)
                ktxt = f"  kernel {kernel_us[k]:.1f} us, {gbs:.0f} GB/s"
            k += 1
            lines.append(f"  {name:11s} fused {ma:.4f} {[round(t, 4) for t in ta]} n={ra}  composition {mb:.4f} {[round(t, 4) for t in tb]} n={rb}  "
                         f"ratio {ma / mb:.4f}{ktxt}  bit-equal {equal}  updated {share:.2f}")
            if name.endswith("+cw") and V == VIEWS[-1] and tag == list(SIZES)[-1]:           # the surface of the last volumes of each grid
                pf, pcmp = (lambda v=vol: tsdf.tsdf_points(v)), (lambda v=vol: points_composition(v))
                got, want = pf(), pcmp()
                pequal = all(same_bits(a, b) for a, b in ((got.xyz, want.xyz), (got.rgb, want.rgb), (got.offsets, want.offsets)))
                pa, pb, qa, qb = alternate(pf, pcmp)
                r[name + " points"] = {"fused_ms": round(median(pa), 4), "fused_runs_ms": [round(t, 4) for t in pa], "composition_ms": round(median(pb), 4),
                                       "composition_runs_ms": [round(t, 4) for t in pb], "ratio": round(median(pa) / median(pb), 4), "bit_equal": pequal,
                                       "points": int(got.xyz.shape[0])}
                lines.append(f"  {name + ' points':18s} tsdf_points {median(pa):.4f} {[round(t, 4) for t in pa]} n={qa}  torch {median(pb):.4f} "
                             f"{[round(t, 4) for t in pb]} n={qb}  ratio {median(pa) / median(pb):.4f}  bit-equal {pequal}  {got.xyz.shape[0]} points")
            del vol, count
        res[key] = r
        lines.append("")
    if args.kernels_only:
        return
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
