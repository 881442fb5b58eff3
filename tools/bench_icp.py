"""Times icp.track_camera / icp.icp_linearize + icp.icp_solve (ud_icp_linearize, ud_icp_update, csrc/icp.hip) against the composition they
fuse -- icp.track_camera_composition / icp.icp_linearize_composition and the solve restated in torch: gt_points, project_camera,
remap(mode="nearest"), about 60 element-wise launches, 30 torch.sum in fp64 and about 400 launches of fp64 scalar arithmetic per step -- on
the GPU box: B = 1 and 8 at 518 x 518 and 480 x 640 (frame and model maps of the same size), time per call in a full queue of calls
(events around each call, median of a window; three windows per arm after a warm-up, the two arms alternating on the same GPU in the same
process).

    pin_pin     a Pinhole frame against the maps of a Pinhole model camera
    eucm_pin    an EUCM frame against the maps of a Pinhole model camera

    step        one icp_linearize and one icp_solve (three launches), windows of 200 calls
    track10     track_camera(iters=10) (twenty launches and the copy of the start), windows of 20 calls

The scene is the smooth surface d(x, y) = 2 + 0.4 sin 2x + 0.3 cos 2.5y + 0.2 x y over the normalised image coordinates, seen by both
cameras from one place; the model maps are its points and analytic normals, the border row and column invalid; the start is 1.8 degrees
and 0.054 away from the identity, the truth; dist_tol 0.1.  Before timing, the fused step's matched, residual and rows are compared with
the composition's bit for bit at the timed size, and the pose after ten steps of both.  The times are events around Python calls on
cache-warm buffers: a CALL RATE, close to the host's submission rate where the kernels are short.  Kernel times come from a run of their
own:
    rocprofv3 --kernel-trace -d DIR -o icp -- python tools/bench_icp.py --kernels-only
which runs, per workload in the order of the table, track_camera(iters=1) 50 times with 256 (the default), 512 and 1024 workgroups per
image and then icp_linearize 50 times (whose second launch only sums); --trace DIR/.../icp_results.db (the profiler's SQLite output) then
adds the median durations of each group's 50 icp_rows_kernel and 50 icp_solve_kernel dispatches and the algorithmic bytes per second of
the first: the depth read once, and for every pixel a byte of model_valid and six floats of the model maps (B * H * W * 29 bytes).
Prints one JSON line and writes the table to --out (default profiles/icp_bench.txt).
    python tools/bench_icp.py [--out PATH] [--kernels-only] [--trace PATH] [--resources TEXT]"""
import argparse
import json
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import gtpoints, icp, unproject  # noqa: E402

REPS, REPS_TRACK, WINDOWS, TRACE_CALLS = 200, 20, 3, 50
PINHOLE, EUCM = 1, 2
SIZES = {"518x518": (518, 518), "480x640": (480, 640)}
BATCHES = (1, 8)
WORKLOADS = ("pin_pin", "eucm_pin")
DIST_TOL = 0.1
BLOCKS = (0, 512, 1024)              # icp._LAUNCH_OPTIONS["blocks"] of the traced groups: the default (256) first
GROUPS = len(BLOCKS) + 1             # and the sum-only second launch of icp_linearize
START = ((0.02, -0.03, 0.015), (0.03, -0.02, 0.04))


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


def alternate(a, b, reps):
    """one warm-up window of each, then WINDOWS windows of each, a b a b ...: ([ms of a], [ms of b])"""
    queue_ms(a, max(reps // 10, 2))
    queue_ms(b, max(reps // 10, 2))
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(queue_ms(a, reps))
        tb.append(queue_ms(b, reps))
    return ta, tb


def median(ts):
    return sorted(ts)[len(ts) // 2]


CAMERAS = {
    PINHOLE: lambda H, W: [1.2 * W, 1.2 * W, W / 2, H / 2],
    EUCM: lambda H, W: [1.1 * W, 1.1 * W, W / 2 - 1, H / 2 + 1, 0.55, 1.05],
}


def camera(model, B, H, W):
    out = torch.zeros(B, 16)
    r = CAMERAS[model](H, W)
    out[:, :len(r)] = torch.tensor(r)
    return gtpoints.PreparedCamera(out.cuda(), (model,) * B)


def surface(cam, B, H, W):
    """the surface through `cam`: (z-depth fp32 [B,1,H,W], points fp32 [B,3,H,W], normals fp32 [B,3,H,W] turned towards the camera)"""
    rays = unproject.get_rays(cam, (B, H, W)).double()
    x, y = rays[:, 0] / rays[:, 2], rays[:, 1] / rays[:, 2]
    d = 2 + 0.4 * torch.sin(2 * x) + 0.3 * torch.cos(2.5 * y) + 0.2 * x * y
    dx, dy = 0.8 * torch.cos(2 * x) + 0.2 * y, -0.75 * torch.sin(2.5 * y) + 0.2 * x
    P = torch.stack([x * d, y * d, d], dim=1)
    # the surface is Z - d(X / Z, Y / Z) = 0: its gradient
    n = torch.stack([-dx / d, -dy / d, 1 + (dx * P[:, 0] + dy * P[:, 1]) / (d * d)], dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    n = torch.where((n * P).sum(dim=1, keepdim=True) > 0, -n, n)
    return d[:, None].float().contiguous(), P.float().contiguous(), n.float().contiguous()


def start(B):
    w, t = (torch.tensor(v, dtype=torch.float64) for v in START)
    a = w / 2
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    R = ((1 - a @ a) * torch.eye(3, dtype=torch.float64) + 2 * torch.outer(a, a) + 2 * K) / (1 + a @ a)
    return torch.cat([R, t[:, None]], dim=1).float().repeat(B, 1, 1).cuda()


def workloads(B, H, W):
    """name -> the arguments of the calls"""
    model = camera(PINHOLE, B, H, W)
    _, mp, mn = surface(model, B, H, W)
    mv = torch.zeros(B, 1, H, W, dtype=torch.bool, device="cuda")
    mv[:, :, 1:-1, 1:-1] = True
    out = {}
    for name, frame in (("pin_pin", PINHOLE), ("eucm_pin", EUCM)):
        cam = camera(frame, B, H, W)
        out[name] = (surface(cam, B, H, W)[0], cam, mp, mn, mv, model, start(B))
    return out


def step_fused(a):
    S = icp.icp_linearize(*a, dist_tol=DIST_TOL)
    return icp.icp_solve(S, a[6])


def step_composition(a):
    S = icp.icp_linearize_composition(*a, dist_tol=DIST_TOL)
    return icp._solve_restated(S, a[6], 0.0, 6)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def configs():
    return [(tag, H, W, B) for tag, (H, W) in SIZES.items() for B in BATCHES]


def trace_medians(path):
    """the kernel trace of a --kernels-only run: the median duration (us) of each consecutive group of TRACE_CALLS dispatches of the two
    kernels -> ([rows], [solve]), GROUPS entries per workload"""
    db = sqlite3.connect(path)
    out = []
    for kernel in ("icp_rows_kernel", "icp_solve_kernel"):
        dur = [r[0] / 1e3 for r in db.execute(f"select duration from kernels where name like '%{kernel}%' order by start")]
        assert len(dur) == TRACE_CALLS * GROUPS * len(configs()) * len(WORKLOADS), (len(dur), "dispatches of", kernel, "in the trace")
        out.append([median(dur[k:k + TRACE_CALLS]) for k in range(0, len(dur), TRACE_CALLS)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="run track_camera(iters=1) 50 times per workload and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="icp_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_icp.py needs a GPU"
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace)
        except (OSError, sqlite3.Error, AssertionError) as e:           # the call times do not depend on the trace
            print(f"bench_icp: kernel trace not used ({e!r})", file=sys.stderr)
    res = {"op": "track_camera (frame-to-model point-to-plane ICP, two launches per step)", "reps": REPS, "reps_track": REPS_TRACK, "windows": WINDOWS}
    lines = ["tools/bench_icp.py on " + torch.cuda.get_device_name(0) + f": ms per call (a call rate), median of a window of queued calls ({REPS} for a step, "
             f"{REPS_TRACK} for ten); {WINDOWS} windows per arm after a warm-up, the fused calls alternating with the composition (gt_points, project_camera,",
             "remap, element-wise torch, torch.sum in fp64, the solve restated in torch fp64); [..] = every window; ratio = fused / composition.",
             "step = icp_linearize + icp_solve; track10 = track_camera(iters=10).",
             "kernels = median icp_rows_kernel + icp_solve_kernel durations of 50 dispatches each in a rocprofv3 --kernel-trace run of its own; GB/s = the "
             "algorithmic bytes of the first (B * H * W * 29) over its time; the sweep repeats both with 512 and 1024 workgroups per image." if kernel_us else "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        lines[-1:] = [args.resources, ""]
    k = 0
    for tag, H, W, B in configs():
        key = f"b{B}_{tag}"
        r = {}
        lines.append(f"{key}  (B = {B}, {H * W} frame pixels per image, model maps of the same size)")
        for name, a in workloads(B, H, W).items():
            if args.kernels_only:
                for blocks in BLOCKS:
                    icp._LAUNCH_OPTIONS["blocks"] = blocks
                    for _ in range(TRACE_CALLS):
                        icp.track_camera(*a, iters=1, dist_tol=DIST_TOL)
                icp._LAUNCH_OPTIONS["blocks"] = 0
                for _ in range(TRACE_CALLS):
                    icp.icp_linearize(*a, dist_tol=DIST_TOL)
                torch.cuda.synchronize()
                continue
            got = icp.icp_linearize(*a, dist_tol=DIST_TOL, return_rows=True)
            want = icp.icp_linearize_composition(*a, dist_tol=DIST_TOL, return_rows=True)
            equal = all(same_bits(x, y) for x, y in zip(got[1:], want[1:]))
            share = float(got[1].float().mean())
            T10, stats = icp.track_camera(*a, iters=10, dist_tol=DIST_TOL)
            Tc10, _ = icp.track_camera_composition(*a, iters=10, dist_tol=DIST_TOL)
            pose_ulp = float(((T10.double() - Tc10.double()).abs() / torch.tensor(2.0 ** -23, dtype=torch.float64)).max())   # in ulp of 1
            away = float((T10 - torch.eye(4, device="cuda")[:3]).abs().max())
            ta, tb = alternate(lambda: step_fused(a), lambda: step_composition(a), REPS)
            tc, td = alternate(lambda: icp.track_camera(*a, iters=10, dist_tol=DIST_TOL), lambda: icp.track_camera_composition(*a, iters=10, dist_tol=DIST_TOL),
                               REPS_TRACK)
            ma, mb, mc, md = median(ta), median(tb), median(tc), median(td)
            rd = lambda ts: [round(t, 4) for t in ts]                    # noqa: E731
            r[name] = {"step_fused_ms": round(ma, 4), "step_fused_runs_ms": rd(ta), "step_composition_ms": round(mb, 4), "step_composition_runs_ms": rd(tb),
                       "step_ratio": round(ma / mb, 4), "track10_fused_ms": round(mc, 4), "track10_fused_runs_ms": rd(tc), "track10_composition_ms": round(md, 4),
                       "track10_composition_runs_ms": rd(td), "track10_ratio": round(mc / md, 4), "rows_bit_equal": equal, "matched_share": round(share, 3),
                       "pose_vs_composition_ulp_of_1": pose_ulp, "pose_error_max_abs": away, "statuses": stats[0, :, 3].tolist()}
            ktxt = ""
            if kernel_us:
                rows_us, solve_us = kernel_us[0][k:k + GROUPS], kernel_us[1][k:k + GROUPS]
                gbs = B * H * W * 29 / (rows_us[0] * 1e-6) / 1e9
                r[name].update(rows_kernel_us=round(rows_us[0], 1), solve_kernel_us=round(solve_us[0], 1), algorithmic_GBps=round(gbs, 1),
                               sum_only_kernel_us=round(solve_us[-1], 1),
                               by_blocks={str(b or 256): [round(rows_us[i], 1), round(solve_us[i], 1)] for i, b in enumerate(BLOCKS)})
                sweep = ", ".join(f"{b or 256}: {rows_us[i]:.1f} + {solve_us[i]:.1f}" for i, b in enumerate(BLOCKS))
                ktxt = f"  kernels {rows_us[0]:.1f} + {solve_us[0]:.1f} us, {gbs:.0f} GB/s (the second launch summing only: {solve_us[-1]:.1f} us; by workgroups per image {sweep})\n{'':10s}"
            k += GROUPS
            lines.append(f"  {name:9s} step fused {ma:.4f} {rd(ta)}  composition {mb:.4f} {rd(tb)}  ratio {ma / mb:.4f}")
            lines.append(f"  {'':9s} track10 fused {mc:.4f} {rd(tc)}  composition {md:.3f} {rd(td)}  ratio {mc / md:.4f}")
            lines.append(f"  {'':9s}{ktxt}  rows bit-equal {equal}  matched {share:.2f}  pose after 10 steps: {pose_ulp:.1f} ulp of 1 from the composition's, "
                         f"{away:.1e} from the identity")
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
