"""Times warp.warp_camera (ud_warp_camera, csrc/warp.hip) against the composition it fuses -- unproject_camera, project_camera, the validity
arithmetic, remap (and remap of the source's depth with the visibility comparison) -- on the GPU box: B = 8 at 518 x 518 and at 480 x 640
(both views), time per call in a full queue of calls (events around each call, median of a window of 200; three windows per arm after a
warm-up, the two arms alternating on the same GPU in the same process).

    pin_pin_u8        Pinhole -> Pinhole from a depth with a per-image transform, C = 3 uint8 -> uint8
    pin_pin_u8_all    the same with src_depth + tolerance and every output (valid, visible, uv, proj_depth)
    eucm_fe_f32       an EUCM destination -> a Fisheye624 source, C = 1 fp32 with a source mask, normalised, with the validity
    points_u8         the points form (a point map instead of depth + camera), Pinhole source, C = 3 uint8
    mixed_src_u8      a Pinhole destination -> a batch of all six source models, C = 3 uint8

Before timing, every output of the fused call is compared with the composition's bit for bit at the timed size.  The times are events
around Python calls on cache-warm buffers: a CALL RATE, close to the host's submission rate where the kernels are short.  Kernel times
come from a run of their own:
    rocprofv3 --kernel-trace -d DIR -o warp -- python tools/bench_warp.py --kernels-only
which launches every fused workload 50 times in the order of the table; --trace DIR/warp_results.db (the profiler's SQLite output) then
adds the median duration of each workload's 50 wp_warp_kernel dispatches to the table.
Prints one JSON line and writes the table to --out (default profiles/warp_bench.txt).
    python tools/bench_warp.py [--out PATH] [--kernels-only] [--trace PATH] [--resources TEXT]"""
import argparse
import json
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import gtpoints, reproject, unproject, warp  # noqa: E402
from unidepth_amd.remap import remap  # noqa: E402

REPS, WINDOWS, TRACE_CALLS = 200, 3, 50
PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI = 1, 2, 3, 4, 5, 6
SIZES = {"b8_518x518": (518, 518), "b8_480x640": (480, 640)}
WORKLOADS = ("pin_pin_u8", "pin_pin_u8_all", "eucm_fe_f32", "points_u8", "mixed_src_u8")
TOL = 0.05


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


def composition(src, *, depth=None, camera=None, points=None, src_camera, transform=None, src_mask=None, normalize=False, src_depth=None,
                occlusion_tol=None):
    """what a caller writes without the fused kernel: (out, valid, visible or None, uv, proj_depth)"""
    Hs, Ws = src.shape[-2:]
    if points is None:
        pts = unproject.unproject_camera(None, camera, depth=depth, image_shape=tuple(depth.shape[-2:]))
    else:
        pts = points
    uv, inside, dproj = reproject.project_camera(pts, src_camera, image_shape=(Hs, Ws), transform=transform)
    cv = inside & (dproj > 0)
    if points is None:
        cv = cv & (depth[:, 0] > 0)
    out, valid = remap(src, uv, src_mask=src_mask, coord_valid=cv, normalize=normalize, return_mask=True)
    visible = None
    if src_depth is not None:
        m = src_depth > 0 if src_mask is None else (src_depth > 0) & src_mask
        ds, dv = remap(src_depth, uv, src_mask=m, coord_valid=cv, normalize=True, return_mask=True)
        visible = dv & ((ds - dproj[:, None]).abs() <= occlusion_tol * dproj[:, None])
    return out, valid, visible, uv, dproj


def rows(models, table, H, W):
    out = torch.zeros(len(models), 16)
    for b, m in enumerate(models):
        r = table[m](H, W)
        out[b, :len(r)] = torch.tensor(r)
    return gtpoints.PreparedCamera(out.cuda(), models)


# a view of about +-30 degrees horizontally for every model
CAMERAS = {
    PINHOLE: lambda H, W: [0.85 * W, 0.85 * W + 1, W / 2 + 1, H / 2 - 1],
    EUCM: lambda H, W: [0.8 * W, 0.8 * W + 1, W / 2 - 1, H / 2 + 1, 0.55, 1.05],
    SPHERICAL: lambda H, W: [1.0, 1.0, W / 2, H / 2, float(W), float(H), 0.55, 0.55 * H / W],
    OPENCV: lambda H, W: [0.85 * W, 0.85 * W + 1, W / 2 + 1, H / 2, -0.22, 0.07, -0.008, 0, 0, 0, 1e-3, -2e-3, 1e-3, 5e-4, -1e-3, 2e-4],
    FISHEYE624: lambda H, W: [0.9 * W, 0.9 * W + 1, W / 2 + 1, H / 2 - 1, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 1e-3, -1e-3, 0, 0, 0, 0],
    MEI: lambda H, W: [1.6 * W, 1.6 * W + 1, W / 2, H / 2 + 1, -0.1, 0.02, 1e-3, -1e-3, 0.9],
}


def workloads(B, H, W):
    """name -> (fused call, composition call), both returning (out, valid, visible, uv, proj_depth) with None for what is not asked for"""
    g = torch.Generator().manual_seed(0)
    depth = (2.0 + 8.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
    depth[:, :, ::17, ::13] = 0.0
    rgb = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8).cuda()
    feat = (5.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
    hole = (torch.rand(B, 1, H, W, generator=g) >= 0.2).cuda()
    sdepth = (2.0 + 8.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
    T = torch.eye(4)[:3].repeat(B, 1, 1)
    T[:, :, 3] = 0.4 * (torch.rand(B, 3, generator=g) - 0.5)
    T[:, 0, 2], T[:, 2, 0] = 0.03, -0.03
    T = T.cuda()
    pin, pin2 = rows((PINHOLE,) * B, CAMERAS, H, W), rows((PINHOLE,) * B, CAMERAS, H, W)
    pin2.params[:, :2] *= 1.1
    eucm, fe = rows((EUCM,) * B, CAMERAS, H, W), rows((FISHEYE624,) * B, CAMERAS, H, W)
    six = rows(tuple((PINHOLE, EUCM, SPHERICAL, OPENCV, FISHEYE624, MEI)[b % 6] for b in range(B)), CAMERAS, H, W)
    points = unproject.unproject_camera(None, pin, depth=depth, image_shape=(H, W))

    def pair(src, flags, **kw):
        """flags: which of (valid, uv, proj_depth) the fused call returns; visible comes with src_depth"""
        mask_, uv_, pd_ = flags
        vis_ = "src_depth" in kw

        def fused():
            res = warp.warp_camera(src, return_mask=mask_, return_uv=uv_, return_depth=pd_, **kw)
            res = list(res) if isinstance(res, tuple) else [res]
            out = [res.pop(0)]
            for have in (mask_, vis_, uv_, pd_):
                out.append(res.pop(0) if have else None)
            return tuple(out)
        return fused, (lambda: composition(src, **kw))
    base = dict(depth=depth, camera=pin, src_camera=pin2, transform=T)
    return {
        "pin_pin_u8": pair(rgb, (False, False, False), **base),
        "pin_pin_u8_all": pair(rgb, (True, True, True), src_depth=sdepth, occlusion_tol=TOL, **base),
        "eucm_fe_f32": pair(feat, (True, False, False), depth=depth, camera=eucm, src_camera=fe, transform=T, src_mask=hole, normalize=True),
        "points_u8": pair(rgb, (False, False, False), points=points, src_camera=pin2, transform=T),
        "mixed_src_u8": pair(rgb, (False, False, False), depth=depth, camera=pin, src_camera=six, transform=T),
    }


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def trace_medians(path):
    """the kernel trace of a --kernels-only run: the median duration (us) of each consecutive group of TRACE_CALLS wp_warp_kernel dispatches"""
    db = sqlite3.connect(path)
    dur = [r[0] / 1e3 for r in db.execute("select duration from kernels where name like '%wp_warp_kernel%' order by start")]
    assert len(dur) == TRACE_CALLS * len(SIZES) * len(WORKLOADS), (len(dur), "dispatches in the trace")
    return [median(dur[k:k + TRACE_CALLS]) for k in range(0, len(dur), TRACE_CALLS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch every fused workload 50 times and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="warp_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_warp.py needs a GPU"
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace)
        except (OSError, sqlite3.Error, AssertionError) as e:           # the call times do not depend on the trace
            print(f"bench_warp: kernel trace not used ({e!r})", file=sys.stderr)
    res = {"op": "warp_camera (backward warping through the camera models, one launch)", "reps": REPS, "windows": WINDOWS}
    lines = ["tools/bench_warp.py on " + torch.cuda.get_device_name(0) + f": ms per call (a call rate), median of a window of {REPS} queued calls; "
             f"{WINDOWS} windows per arm after a warm-up, the fused call alternating with the composition (unproject_camera, project_camera,",
             "the validity arithmetic, remap [, remap of src_depth and the comparison]); [..] = every window; ratio = fused / composition.",
             "kernel = median wp_warp_kernel duration of 50 dispatches in a rocprofv3 --kernel-trace run of its own." if kernel_us else
             "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        lines[-1:] = [args.resources, ""]
    B, k = 8, 0
    for tag, (H, W) in SIZES.items():
        r = {}
        lines.append(f"{tag}  (B = {B}, {H * W} destination pixels per image, source of the same size)")
        for name, (fused, comp) in workloads(B, H, W).items():
            if args.kernels_only:
                for _ in range(TRACE_CALLS):
                    fused()
                torch.cuda.synchronize()
                continue
            got, want = fused(), comp()
            equal = all(g is None or same_bits(g, w) for g, w in zip(got, want))
            share = float(want[1].float().mean())
            ta, tb = alternate(fused, comp)
            ma, mb = median(ta), median(tb)
            r[name] = {"fused_ms": round(ma, 4), "fused_runs_ms": [round(t, 4) for t in ta], "composition_ms": round(mb, 4),
                       "composition_runs_ms": [round(t, 4) for t in tb], "ratio": round(ma / mb, 3), "bit_equal": equal, "valid_share": round(share, 3)}
            ktxt = ""
            if kernel_us:
                r[name]["kernel_us"] = round(kernel_us[k], 1)
                ktxt = f"  kernel {kernel_us[k]:.1f} us"
            k += 1
            lines.append(f"  {name:15s} fused {ma:.4f} {[round(t, 4) for t in ta]}  composition {mb:.4f} {[round(t, 4) for t in tb]}  ratio {ma / mb:.3f}"
                         f"{ktxt}  bit-equal {equal}  valid {share:.2f}")
        res[tag] = r
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
