"""Times the surface normals and their metrics (unidepth_amd/normals.py, csrc/normals.hip) against what a caller writes without them, on
the GPU box: B = 8 at 518 x 518 and at 480 x 640, time per call in a full queue of calls (events around each call, median of a window of
200; three windows per arm after a warm-up, the arms alternating on the same GPU in the same process).

    points            normals_from_points (mask, depth, edge_rtol, all outputs) against the torch composition of the same definition
    camera_pinhole    normals_camera, all Pinhole, against gt_points + normals_from_points
    camera_eucm       the same, all EUCM
    camera_mixed      the same, the four closed-form models in turn
    eval              eval_normals against a torch loop (acos, median and the means per image, read back once per call)

Before timing, every output of normals_camera is compared with the composition's bit for bit at the timed size.  The times are events
around Python calls on cache-warm buffers: a CALL RATE, close to the host's submission rate where the kernels are short.  Kernel times
come from a run of their own:
    rocprofv3 --kernel-trace -d DIR -o normals -- python tools/bench_normals.py --kernels-only
which launches every timed HIP workload 50 times in the order of the table; --trace DIR/normals_results.db (the profiler's SQLite output)
then adds the median duration of each workload's dispatches and the fraction of the HBM peak its algorithmic traffic reaches.
--alt-lib PATH names a second build of the library with -DUD_NM_RECOMPUTE (csrc/build.sh -DUD_NM_RECOMPUTE with UD_OUT=PATH), whose depth
kernel reconstructs five points per pixel instead of staging a tile with its halo in LDS: two more arms of the camera_* workloads: this build's
and that build's ud_normals called through the C-ABI on one descriptor, in the same process.
Prints one JSON line and writes the table to --out (default profiles/normals_bench.txt).
    python tools/bench_normals.py [--out PATH] [--kernels-only] [--trace PATH] [--alt-lib PATH] [--resources TEXT]"""
import argparse
import ctypes as C
import json
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import _args, _lib, gtpoints, normals  # noqa: E402
from unidepth_amd.ops import check, cur_stream, mk  # noqa: E402

REPS, WINDOWS, TRACE_CALLS = 200, 3, 50
PINHOLE, EUCM, SPHERICAL, MEI = 1, 2, 3, 6
SIZES = {"b8_518x518": (518, 518), "b8_480x640": (480, 640)}
WORKLOADS = ("points", "camera_pinhole", "camera_eucm", "camera_mixed", "eval")
KERNEL_OF = {"points": "nm_points_kernel", "camera_pinhole": "nm_depth_kernel", "camera_eucm": "nm_depth_kernel", "camera_mixed": "nm_depth_kernel"}
# algorithmic bytes per pixel: points 12 + depth 4 + mask 1 in, normals 12 + valid 1 + rgb 3 out; the depth form reads 4 + 1 instead of 17
BYTES_PER_PIXEL = {"points": 33, "camera_pinhole": 21, "camera_eucm": 21, "camera_mixed": 21}
EVAL_LAUNCHES = 9                                   # zero, stats, select, 3 x (digit, select)
HBM_PEAK = 8.0e12                                   # bytes / s, the MI355X datasheet figure
EDGE = 0.05
CAMERAS = {
    PINHOLE: lambda H, W: [0.85 * W, 0.85 * W + 1, W / 2 + 1, H / 2 - 1],
    EUCM: lambda H, W: [0.8 * W, 0.8 * W + 1, W / 2 - 1, H / 2 + 1, 0.55, 1.05],
    SPHERICAL: lambda H, W: [1.0, 1.0, W / 2, H / 2, float(W), float(H), 0.55, 0.55 * H / W],
    MEI: lambda H, W: [1.6 * W, 1.6 * W + 1, W / 2, H / 2 + 1, -0.1, 0.02, 1e-3, -1e-3, 0.9],
}


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


def alternate(fns):
    """one warm-up window of each, then WINDOWS windows of each, a b c a b c ...: [[ms of a], [ms of b], ...]"""
    for f in fns:
        queue_ms(f, 20)
    ts = [[] for _ in fns]
    for _ in range(WINDOWS):
        for k, f in enumerate(fns):
            ts[k].append(queue_ms(f))
    return ts


def median(ts):
    return sorted(ts)[len(ts) // 2]


def rows(models, H, W):
    out = torch.zeros(len(models), 16)
    for b, m in enumerate(models):
        r = CAMERAS[m](H, W)
        out[b, :len(r)] = torch.tensor(r)
    return gtpoints.PreparedCamera(out.cuda(), models)


def torch_normals(P, mask, depth, rtol):
    """the definition of normals_from_points in torch ops (rolls, masks, a cross product, two normalisations, the orientation, the bytes)"""
    ok = mask.bool()[:, 0] & torch.isfinite(P).all(dim=1)
    use, pts = {}, {}
    for name, (dim, sh) in dict(L=(2, 1), R=(2, -1), U=(1, 1), D=(1, -1)).items():
        u = torch.roll(ok, sh, dims=dim)
        dq = torch.roll(depth[:, 0], sh, dims=dim)
        idx = 0 if sh == 1 else -1
        if dim == 2:
            u[:, :, idx] = False
        else:
            u[:, idx, :] = False
        u = u & ((depth[:, 0] - dq).abs() <= rtol * torch.minimum(depth[:, 0], dq))
        use[name], pts[name] = u, torch.roll(P, sh, dims=dim + 1)
    dx = torch.where(use["R"][:, None], pts["R"], P) - torch.where(use["L"][:, None], pts["L"], P)
    dy = torch.where(use["D"][:, None], pts["D"], P) - torch.where(use["U"][:, None], pts["U"], P)
    n = torch.cross(dy, dx, dim=1)
    m = n.abs().amax(dim=1)
    valid = ok & (use["L"] | use["R"]) & (use["U"] | use["D"]) & (m > 0) & torch.isfinite(m)
    n = n / m[:, None]
    n = n / n.norm(dim=1, keepdim=True)
    n = torch.where(((n * P).sum(dim=1) > 0)[:, None], -n, n)
    n = torch.where(valid[:, None], n, torch.zeros_like(n))
    rgb = torch.where(valid[:, None], torch.floor((n + 1) * 127.5 + 0.5).clamp(0, 255), torch.zeros_like(n)).to(torch.uint8)
    return n, valid[:, None], rgb


def torch_eval(gt, pred, mask):
    """a torch loop over the images: acos of the normalised dot, the mean, the median, the rmse and three shares, read back once"""
    out = []
    for b in range(gt.shape[0]):
        g, p = gt[b].reshape(3, -1), pred[b].reshape(3, -1)
        lg, lp = g.norm(dim=0), p.norm(dim=0)
        keep = mask[b].reshape(-1).bool() & (lg > 0) & (lp > 0)
        e = torch.rad2deg(torch.acos(((g * p).sum(dim=0) / (lg * lp)).clamp(-1, 1)))[keep]
        out.append(torch.stack([e.mean(), e.median(), (e * e).mean().sqrt(), (e < 11.25).float().mean(), (e < 22.5).float().mean(),
                                (e < 30.0).float().mean()]))
    return torch.stack(out)


def alt_depth_call(alt, depth, cam, mask, out):
    """ud_normals of a second build of the library on the same descriptor (the depth form, all outputs)"""
    B, _, H, W = depth.shape
    d = mk(_lib.UdNormals, points=None, depth=depth, params=cam.params, mask=mask.view(torch.uint8), normals=out[0], valid=out[1], rgb=out[2],
           B=B, H=H, W=W, mask_shared=0, has_rtol=1, rtol_bits=_args.f32_bits(EDGE))
    for b in range(B):
        d.model[b] = cam.models[b]

    def call():
        check(alt.ud_normals(C.byref(d), C.c_void_p(cur_stream())), "ud_normals (alt)")
        return out
    return call


def workloads(B, H, W, alt):
    """name -> [the HIP call, what it replaces, (the raw C-ABI call of this build and of the alternative build)]"""
    g = torch.Generator().manual_seed(0)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = (2.0 + 0.6 * x / W + 0.9 * y / H + 0.002 * torch.randn(B, 1, H, W, generator=g))
    depth[:, :, H // 4:3 * H // 4, W // 3:2 * W // 3] *= 0.6
    depth[:, :, ::17, ::13] = 0.0
    depth = depth.cuda()
    mask = (torch.rand(B, 1, H, W, generator=g) >= 0.1).cuda()
    cams = {"camera_pinhole": rows((PINHOLE,) * B, H, W), "camera_eucm": rows((EUCM,) * B, H, W),
            "camera_mixed": rows(tuple((PINHOLE, EUCM, SPHERICAL, MEI)[b % 4] for b in range(B)), H, W)}
    pts = gtpoints.gt_points(depth, cams["camera_pinhole"])
    eff = mask & (depth > 0)
    kw = dict(edge_rtol=EDGE, return_mask=True, return_rgb=True)
    w = {"points": [lambda: normals.normals_from_points(pts, mask=eff, depth=depth, **kw), lambda: torch_normals(pts, eff, depth, EDGE)]}
    for name, cam in cams.items():
        def fused(cam=cam):
            return normals.normals_camera(depth, cam, mask=mask, **kw)

        def comp(cam=cam):
            return normals.normals_from_points(gtpoints.gt_points(depth, cam), mask=mask & (depth > 0), depth=depth, **kw)
        w[name] = [fused, comp]
        if alt is not None:
            out = (torch.empty(B, 3, H, W, device="cuda"), torch.empty(B, 1, H, W, device="cuda", dtype=torch.uint8),
                   torch.empty(B, 3, H, W, device="cuda", dtype=torch.uint8))
            w[name] += [alt_depth_call(_lib.lib, depth, cam, mask, out), alt_depth_call(alt, depth, cam, mask, out)]
    gt = normals.normals_camera(depth, cams["camera_mixed"], mask=mask)
    pred = normals.normals_camera(depth + 0.02 * torch.randn(B, 1, H, W, generator=g).cuda(), cams["camera_mixed"], mask=mask)
    w["eval"] = [lambda: normals.eval_normals(gt, pred, mask), lambda: torch_eval(gt, pred, mask).cpu()]
    return w


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    if a.dtype == torch.bool:
        a = a.view(torch.uint8)
    if b.dtype == torch.bool:
        b = b.view(torch.uint8)
    return a.shape == b.shape and bool(torch.equal(a, b))


def trace_medians(path):
    """the kernel trace of a --kernels-only run -> {(size tag, workload): us}: the median duration of each consecutive group of TRACE_CALLS
    dispatches of the workload's kernel; for eval, the sum of the medians of its nine launches"""
    db = sqlite3.connect(path)
    ours = ("nm_points_kernel", "nm_depth_kernel", "en_zero_kernel", "en_stats_kernel", "en_select_kernel", "en_digit_kernel")
    rows_ = [(n, d / 1e3) for n, d in db.execute("select name, duration from kernels order by start") if any(k in n for k in ours)]
    out, at = {}, 0
    for tag in SIZES:
        assert all("nm_depth_kernel" in n for n, _ in rows_[at:at + 2]), tag       # workloads() makes eval's inputs with two calls
        at += 2
        for name in WORKLOADS:
            per_call = EVAL_LAUNCHES if name == "eval" else 1
            chunk = rows_[at:at + TRACE_CALLS * per_call]
            at += TRACE_CALLS * per_call
            assert len(chunk) == TRACE_CALLS * per_call, (tag, name, len(chunk))
            if name == "eval":
                assert all(("en_" in n) for n, _ in chunk), (tag, name)
                out[(tag, name)] = sum(median([chunk[c * per_call + k][1] for c in range(TRACE_CALLS)]) for k in range(per_call))
            else:
                assert all(KERNEL_OF[name] in n for n, _ in chunk), (tag, name, chunk[0][0])
                out[(tag, name)] = median([d for _, d in chunk])
    assert at == len(rows_), (at, len(rows_))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch every HIP workload 50 times and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="normals_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--alt-lib", default=None, help="a build of the library with -DUD_NM_RECOMPUTE: two more arms of the camera_* workloads")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_normals.py needs a GPU"
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace)
        except (OSError, sqlite3.Error, AssertionError) as e:           # the call times do not depend on the trace
            print(f"bench_normals: kernel trace not used ({e!r})", file=sys.stderr)
    alt = None
    if args.alt_lib and not args.kernels_only:
        alt = C.CDLL(args.alt_lib)
        alt.ud_normals.argtypes, alt.ud_normals.restype = [C.POINTER(_lib.UdNormals), C.c_void_p], C.c_int
    res = {"op": "normals_from_points / normals_camera / eval_normals", "reps": REPS, "windows": WINDOWS}
    lines = ["tools/bench_normals.py on " + torch.cuda.get_device_name(0) + f": ms per call (a call rate), median of a window of {REPS} queued calls; "
             f"{WINDOWS} windows per arm after a warm-up, the arms alternating; [..] = every window; ratio = hip / replaced.",
             "points: normals_from_points vs the torch composition of the same definition.  camera_*: normals_camera (the LDS-halo kernel) vs gt_points +",
             "normals_from_points" + ("; raw C-ABI call: ud_normals of this build and of the recompute-five build (-DUD_NM_RECOMPUTE) on one descriptor." if alt else ".") +
             "  eval: eval_normals vs a torch loop read back once per call.",
             "kernel = median duration of 50 dispatches in a rocprofv3 --kernel-trace run of its own (eval: the sum over its 9 launches); hbm = algorithmic "
             "bytes / kernel time / 8 TB/s." if kernel_us else "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        lines[-1:] = [args.resources, ""]
    B = 8
    for tag, (H, W) in SIZES.items():
        r = {}
        lines.append(f"{tag}  (B = {B}, {H * W} pixels per image)")
        for name, fns in workloads(B, H, W, alt).items():
            if args.kernels_only:
                for _ in range(TRACE_CALLS):
                    fns[0]()
                torch.cuda.synchronize()
                continue
            equal = None
            if name.startswith("camera"):
                got = [fn() for fn in fns]
                equal = all(same_bits(g, w_) for other in got[1:] for g, w_ in zip(got[0], other))
            ts = alternate(fns)
            ms = [median(t) for t in ts]
            r[name] = {"hip_ms": round(ms[0], 4), "hip_runs_ms": [round(t, 4) for t in ts[0]], "replaced_ms": round(ms[1], 4),
                       "replaced_runs_ms": [round(t, 4) for t in ts[1]], "ratio": round(ms[0] / ms[1], 3)}
            txt = f"  {name:15s} hip {ms[0]:.4f} {[round(t, 4) for t in ts[0]]}  replaced {ms[1]:.4f} {[round(t, 4) for t in ts[1]]}  ratio {ms[0] / ms[1]:.3f}"
            if len(fns) > 2:                            # the two forms of the depth kernel on one descriptor, without the Python surface
                r[name].update(raw_lds_ms=round(ms[2], 4), raw_lds_runs_ms=[round(t, 4) for t in ts[2]], raw_recompute_ms=round(ms[3], 4),
                               raw_recompute_runs_ms=[round(t, 4) for t in ts[3]])
                txt += f"  raw C-ABI call: lds-halo {ms[2]:.4f} {[round(t, 4) for t in ts[2]]}  recompute-five {ms[3]:.4f} {[round(t, 4) for t in ts[3]]}"
            if equal is not None:
                r[name]["bit_equal"] = equal
                txt += f"  bit-equal {equal}"
            if kernel_us:
                us = kernel_us[(tag, name)]
                r[name]["kernel_us"] = round(us, 1)
                txt += f"  kernel {us:.1f} us"
                if name in BYTES_PER_PIXEL:
                    frac = BYTES_PER_PIXEL[name] * B * H * W / (us * 1e-6) / HBM_PEAK
                    r[name]["hbm_fraction"] = round(frac, 3)
                    txt += f"  hbm {frac:.2f}"
            lines.append(txt)
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
