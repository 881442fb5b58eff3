"""Times unproject.unproject_camera (ud_camera_unproject, csrc/unproject.hip) on the GPU box: B = 8 at 480 x 640 and at 518 x 518,
time per call in a full queue of calls (events around each call, median of a window; three windows, alternating with the counterpart on
the same GPU in the same process), for an all-Pinhole batch, an all-EUCM batch and a mixed batch with two OPENCV and two Fisheye624
members (plus Pinhole, EUCM, Spherical, MEI), each on the identity grid (uv = None) and on [B,N,2] rows of the same count.

    raw rays, closed-form batches     counterpart: the torch composition of the same definitions, what a user writes without the kernel
    identity grid with a depth        counterpart: gtpoints.gt_points, the same arithmetic and output.  On the mixed batch gt_points is
                                      the init / 10 steps / final form (12 launches and a float4 state per pixel), unproject_camera the
                                      two-pass form (2 launches, no state): this is the comparison of the two.

Launches per call are those the host code enqueues (with an OPENCV / Fisheye624 member the maxima are cleared first: a small launch in
unproject_camera, a memset node in gt_points).
Camera rows are uploaded once (prepare_camera).  The times are events around Python calls on cache-warm buffers: a call rate, which at
these sizes is close to the host's submission rate for the closed-form batches; no kernel trace is taken here and no bandwidth is derived.
Prints one JSON line and writes the table to --out (default profiles/unproject_bench.txt).
    python tools/bench_unproject.py [--out PATH]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import cameras, gtpoints, unproject  # noqa: E402

REPS, WINDOWS = 200, 3


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
    """WINDOWS windows of each, a b a b ...: ([ms of a], [ms of b])"""
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(queue_ms(a))
        tb.append(queue_ms(b))
    return ta, tb


def torch_pinhole(u, v, p, dim):
    """((u - cx) / fx, (v - cy) / fy, 1) / max(z, 1e-4) in torch: p a list of parameter columns shaped to broadcast against u, v"""
    fx, fy, cx, cy = p[:4]
    x, y = (u - cx) / fx, (v - cy) / fy
    x, y = torch.broadcast_tensors(x, y)
    r = torch.stack([x, y, torch.ones_like(x)], dim)
    return r / r.narrow(dim, 2, 1).clamp(min=1e-4)


def torch_eucm(u, v, p, dim):
    """the EUCM row of the definition table in torch"""
    fx, fy, cx, cy, al, be = p[:6]
    mx, my = torch.broadcast_tensors((u - cx) / fx, (v - cy) / fy)
    r2 = mx * mx + my * my
    mz = (1 - be * al * al * r2) / (al * torch.sqrt((1 - (2 * al - 1) * be * r2).clamp(min=1e-5)) + (1 - al))
    c = 1 / torch.sqrt(mx * mx + my * my + mz * mz + 1e-5)
    return torch.stack([c * mx, c * my, (c * mz).clamp(min=1e-3)], dim)


def summary(ts):
    return round(sorted(ts)[len(ts) // 2], 4), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unproject_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_unproject.py needs a GPU"
    res = {"op": "unproject_camera (Camera.unproject of a batch at any image coordinate, one camera model per image)", "reps": REPS, "windows": WINDOWS}
    lines = ["tools/bench_unproject.py on " + torch.cuda.get_device_name(0) + f": ms per call, median of a window of {REPS} queued calls; "
             f"{WINDOWS} windows per arm, alternating with the counterpart; [..] = every window.  No kernel trace was taken.", ""]
    B = 8
    for tag, (H, W) in {"b8_480x640": (480, 640), "b8_518x518": (518, 518)}.items():
        N = H * W
        g = torch.Generator().manual_seed(0)
        depth = (0.5 + 40.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
        rows = (torch.rand(B, N, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32)).cuda()
        f = 0.8 * W
        j = torch.arange(B, dtype=torch.float32)
        pin = torch.stack([f + j, f + 2 * j, W / 2 + 0.3 * j, H / 2 - 0.2 * j], 1)
        euc = torch.cat([pin, torch.stack([0.4 + 0.03 * j, 1.0 + 0.02 * j], 1)], 1)
        ocv = [f, f + 1, W / 2 + 1, H / 2 - 1, -0.25, 0.08, -0.01, 0, 0, 0, 1e-3, -2e-3, 1e-3, 5e-4, -1e-3, 2e-4]
        fe = [0.4 * W, 0.4 * W + 1, W / 2 + 1, H / 2 - 1, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 1e-3, -1e-3, 0, 0, 0, 0]
        mixed = cameras.BatchCamera([
            cameras.OPENCV(torch.tensor(ocv)), cameras.Pinhole(params=pin[1:2]), cameras.Fisheye624(torch.tensor(fe)), cameras.EUCM(euc[3:4]),
            cameras.OPENCV(torch.tensor(ocv[:4] + [-0.1, 0.02] + ocv[6:])), cameras.Spherical(torch.tensor([f, f, W / 2, H / 2, float(W), float(H), 3.1, 1.5])),
            cameras.Fisheye624(torch.tensor(fe[:4] + [0.02, 0.004] + fe[6:])), cameras.MEI(torch.tensor([f, f, W / 2, H / 2, -0.1, 0.02, 1e-3, -1e-3, 0.9]))])
        cams = {"pinhole": gtpoints.prepare_camera(cameras.Pinhole(params=pin), B, "cuda"),
                "eucm": gtpoints.prepare_camera(cameras.EUCM(euc), B, "cuda"),
                "mixed_2opencv_2fisheye": gtpoints.prepare_camera(mixed, B, "cuda")}
        torch_fns = {"pinhole": (torch_pinhole, pin.cuda()), "eucm": (torch_eucm, euc.cuda())}
        gu = (torch.arange(W, device="cuda", dtype=torch.float32) + 0.5).view(1, 1, W)
        gv = (torch.arange(H, device="cuda", dtype=torch.float32) + 0.5).view(1, H, 1)
        r = {}
        lines.append(f"{tag}  (B = {B}, {N} points per image)")
        for name, cam in cams.items():
            iterative = name.startswith("mixed")
            launches = {"unproject": "clear + 2" if iterative else "1", "gt_points": "memset + 12" if iterative else "1"}
            grid_fn = lambda: unproject.unproject_camera(None, cam, image_shape=(H, W))          # noqa: E731
            rows_fn = lambda: unproject.unproject_camera(rows, cam)                              # noqa: E731
            if name in torch_fns:
                fn, p = torch_fns[name]
                pg = [p[:, i].view(B, 1, 1) for i in range(p.shape[1])]
                pr = [p[:, i].view(B, 1) for i in range(p.shape[1])]
                tgrid_fn = lambda: fn(gu, gv, pg, 1)                                              # noqa: E731
                trows_fn = lambda: fn(rows[..., 0], rows[..., 1], pr, 2)                          # noqa: E731
                r[name + "_grid_max_abs_diff_vs_torch"] = float((grid_fn() - tgrid_fn()).abs().max())
                r[name + "_rows_max_abs_diff_vs_torch"] = float((rows_fn() - trows_fn()).abs().max())
                for what, a, b in (("grid", grid_fn, tgrid_fn), ("rows", rows_fn, trows_fn)):
                    ta, tb = alternate(a, b)
                    (r[f"{name}_{what}_ms"], r[f"{name}_{what}_runs_ms"]), (r[f"{name}_{what}_torch_ms"], r[f"{name}_{what}_torch_runs_ms"]) = summary(ta), summary(tb)
                    lines.append(f"  {name:24s} raw, {what:4s}  unproject_camera {summary(ta)[0]:.4f} {summary(ta)[1]}  torch {summary(tb)[0]:.4f} {summary(tb)[1]}  "
                                 f"launches {launches['unproject']}")
            else:
                ta, tb = alternate(grid_fn, rows_fn)
                (r[name + "_grid_ms"], r[name + "_grid_runs_ms"]), (r[name + "_rows_ms"], r[name + "_rows_runs_ms"]) = summary(ta), summary(tb)
                lines.append(f"  {name:24s} raw, grid  unproject_camera {summary(ta)[0]:.4f} {summary(ta)[1]}  launches {launches['unproject']}")
                lines.append(f"  {name:24s} raw, rows  unproject_camera {summary(tb)[0]:.4f} {summary(tb)[1]}  launches {launches['unproject']}")
            depth_fn = lambda: unproject.unproject_camera(None, cam, depth=depth, image_shape=(H, W))    # noqa: E731
            gt_fn = lambda: gtpoints.gt_points(depth, cam)                                                # noqa: E731
            r[name + "_depth_bit_equal_to_gt_points"] = bool(torch.equal(depth_fn().view(torch.int32), gt_fn().view(torch.int32)))
            ta, tb = alternate(depth_fn, gt_fn)
            (r[name + "_depth_ms"], r[name + "_depth_runs_ms"]), (r[name + "_gt_points_ms"], r[name + "_gt_points_runs_ms"]) = summary(ta), summary(tb)
            form = "two-pass" if iterative else "one launch"
            other = "init / 10 steps / final" if iterative else "one launch"
            lines.append(f"  {name:24s} grid + depth  unproject_camera ({form}, launches {launches['unproject']}) {summary(ta)[0]:.4f} {summary(ta)[1]}  "
                         f"gt_points ({other}, launches {launches['gt_points']}) {summary(tb)[0]:.4f} {summary(tb)[1]}  "
                         f"bit-equal {r[name + '_depth_bit_equal_to_gt_points']}")
        res[tag] = r
        lines.append("")
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
