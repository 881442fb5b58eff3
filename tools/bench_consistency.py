"""Times consistency.depth_consistency (ud_depth_consistency, csrc/consistency.hip) against the composition it fuses --
consistency.depth_consistency_composition: per view warp_camera, unproject_camera, project_camera and the element-wise comparisons -- on
the GPU box: B = 1 and 8, V = 4 and 8 views, 518 x 518 and 480 x 640 (all views), time per call in a full queue of calls (events around
each call, median of a window of 200; three windows per arm after a warm-up, the two arms alternating on the same GPU in the same process).

    pin_pin     a Pinhole reference against Pinhole views
    eucm_pin    an EUCM reference against Pinhole views
    mixed       a Pinhole reference against views cycling through Pinhole, EUCM, Spherical and MEI

The scene is the plane z = 5 seen by views translated sideways, a tenth of every view's pixels pushed 10 % off the plane and a twentieth
empty.  Before timing, every output of the fused call (fused, count, mask) is compared with the composition's bit for bit at the timed
size.  The times are events around Python calls on cache-warm buffers: a CALL RATE, close to the host's submission rate where the kernels
are short.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace -d DIR -o consistency -- python tools/bench_consistency.py --kernels-only
which launches every fused workload 50 times in the order of the table; --trace DIR/consistency_results.db (the profiler's SQLite output)
then adds the median duration of each workload's 50 cs_consistency_kernel dispatches and the algorithmic bytes per second: the reference
depth read once, every view's depth read once, fused + count + mask written once (B * (10 * H * W + 4 * V * Hs * Ws) bytes).
Prints one JSON line and writes the table to --out (default profiles/consistency_bench.txt).
    python tools/bench_consistency.py [--out PATH] [--kernels-only] [--trace PATH] [--resources TEXT]"""
import argparse
import json
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import consistency, gtpoints, unproject  # noqa: E402

REPS, WINDOWS, TRACE_CALLS = 200, 3, 50
PINHOLE, EUCM, SPHERICAL, MEI = 1, 2, 3, 6
SIZES = {"518x518": (518, 518), "480x640": (480, 640)}
BATCHES, VIEWS = (1, 8), (4, 8)
WORKLOADS = ("pin_pin", "eucm_pin", "mixed")
PLANE = 5.0


def queue_ms(fn, reps=REPS):
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


def alternate(a, b):
    """one warm-up window of each, then WINDOWS windows of each, a b a b ...: ([ms of a], [ms of b])"""
    queue_ms(a, 20)
    queue_ms(b, 20)
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(queue_ms(a))
        tb.append(queue_ms(b))
    return ta, tb


def median(ts):
    return sorted(ts)[len(ts) // 2]


# a view of about +-30 degrees horizontally for every model
CAMERAS = {
    PINHOLE: lambda H, W: [0.85 * W, 0.85 * W + 1, W / 2 + 1, H / 2 - 1],
    EUCM: lambda H, W: [0.8 * W, 0.8 * W + 1, W / 2 - 1, H / 2 + 1, 0.55, 1.05],
    SPHERICAL: lambda H, W: [1.0, 1.0, W / 2, H / 2, float(W), float(H), 0.55, 0.55 * H / W],
    MEI: lambda H, W: [1.6 * W, 1.6 * W + 1, W / 2, H / 2 + 1, -0.1, 0.02, 1e-3, -1e-3, 0.9],
}


def camera(model, B, H, W):
    out = torch.zeros(B, 16)
    r = CAMERAS[model](H, W)
    out[:, :len(r)] = torch.tensor(r)
    return gtpoints.PreparedCamera(out.cuda(), (model,) * B)


def plane_depth(cam, B, H, W):
    """the depth map of the plane z = PLANE through `cam`: PLANE for the models whose depth is z, PLANE / ray.z for Spherical's distance"""
    if cam.models[0] != SPHERICAL:
        return torch.full((B, H, W), PLANE, device="cuda")
    return PLANE / unproject.get_rays(cam, (B, H, W))[:, 2]


def workloads(B, V, H, W):
    """name -> (fused call, composition call), both returning (fused, count, mask)"""
    g = torch.Generator().manual_seed(0)
    T = torch.eye(4)[:3].repeat(B, V, 1, 1)
    T[..., :2, 3] = 0.6 * (torch.rand(B, V, 2, generator=g) - 0.5)              # sideways: the plane keeps its z in every view
    T = T.cuda()
    noise = torch.rand(B, V, H, W, generator=g).cuda()
    out = {}
    for name, ref, views in (("pin_pin", PINHOLE, (PINHOLE,)), ("eucm_pin", EUCM, (PINHOLE,)), ("mixed", PINHOLE, (PINHOLE, EUCM, SPHERICAL, MEI))):
        cam = camera(ref, B, H, W)
        cams = [camera(views[v % len(views)], B, H, W) for v in range(V)]
        depth = plane_depth(cam, B, H, W)[:, None].contiguous()
        src = torch.stack([plane_depth(c, B, H, W) for c in cams], dim=1)
        src = torch.where(noise < 0.1, 1.1 * src, src)
        src = torch.where(noise > 0.95, torch.zeros_like(src), src).contiguous()
        args = (depth, cam, src, cams, T)
        out[name] = ((lambda a=args: consistency.depth_consistency(*a)), (lambda a=args: consistency.depth_consistency_composition(*a)))
    return out


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def configs():
    return [(tag, H, W, B, V) for tag, (H, W) in SIZES.items() for B in BATCHES for V in VIEWS]


def trace_medians(path):
    """the kernel trace of a --kernels-only run: the median duration (us) of each consecutive group of TRACE_CALLS cs_consistency_kernel dispatches"""
    db = sqlite3.connect(path)
    dur = [r[0] / 1e3 for r in db.execute("select duration from kernels where name like '%cs_consistency_kernel%' order by start")]
    assert len(dur) == TRACE_CALLS * len(configs()) * len(WORKLOADS), (len(dur), "dispatches in the trace")
    return [median(dur[k:k + TRACE_CALLS]) for k in range(0, len(dur), TRACE_CALLS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch every fused workload 50 times and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="consistency_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_consistency.py needs a GPU"
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace)
        except (OSError, sqlite3.Error, AssertionError) as e:           # the call times do not depend on the trace
            print(f"bench_consistency: kernel trace not used ({e!r})", file=sys.stderr)
    res = {"op": "depth_consistency (multi-view depth check and fusion, one launch)", "reps": REPS, "windows": WINDOWS}
    lines = ["tools/bench_consistency.py on " + torch.cuda.get_device_name(0) + f": ms per call (a call rate), median of a window of {REPS} queued calls; "
             f"{WINDOWS} windows per arm after a warm-up, the fused call alternating with depth_consistency_composition (per view: warp_camera,",
             "unproject_camera, project_camera and the element-wise comparisons); [..] = every window; ratio = fused / composition.",
             "kernel = median cs_consistency_kernel duration of 50 dispatches in a rocprofv3 --kernel-trace run of its own; GB/s = the algorithmic bytes "
             "(B * (10 * H * W + 4 * V * Hs * Ws)) over that time." if kernel_us else "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        lines[-1:] = [args.resources, ""]
    k = 0
    for tag, H, W, B, V in configs():
        key = f"b{B}_v{V}_{tag}"
        r = {}
        lines.append(f"{key}  (B = {B}, V = {V}, {H * W} reference pixels per image, views of the same size)")
        for name, (fused, comp) in workloads(B, V, H, W).items():
            if args.kernels_only:
                for _ in range(TRACE_CALLS):
                    fused()
                torch.cuda.synchronize()
                continue
            got, want = fused(), comp()
            equal = all(same_bits(a, b) for a, b in zip(got, want))
            share = float(got[1].float().mean()) / V
            ta, tb = alternate(fused, comp)
            ma, mb = median(ta), median(tb)
            r[name] = {"fused_ms": round(ma, 4), "fused_runs_ms": [round(t, 4) for t in ta], "composition_ms": round(mb, 4),
                       "composition_runs_ms": [round(t, 4) for t in tb], "ratio": round(ma / mb, 3), "bit_equal": equal, "consistent_share": round(share, 3)}
            ktxt = ""
            if kernel_us:
                gbs = B * (10 * H * W + 4 * V * H * W) / (kernel_us[k] * 1e-6) / 1e9
                r[name]["kernel_us"], r[name]["algorithmic_GBps"] = round(kernel_us[k], 1), round(gbs, 1)
                ktxt = f"  kernel {kernel_us[k]:.1f} us, {gbs:.0f} GB/s"
            k += 1
            lines.append(f"  {name:9s} fused {ma:.4f} {[round(t, 4) for t in ta]}  composition {mb:.4f} {[round(t, 4) for t in tb]}  ratio {ma / mb:.3f}"
                         f"{ktxt}  bit-equal {equal}  consistent {share:.2f}")
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
