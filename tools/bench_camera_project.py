"""Times reproject.project_camera (ud_camera_project, csrc/project.hip) and reproject.render_depth_camera (ud_splat_camera,
csrc/splat.hip) next to the torch composition of the same definitions, on the same GPU, same process, alternating: B = 8 point maps at
518 x 518 and 480 x 640 (gt_points of a smooth depth map through the batch's own cameras, seen through those cameras again), for an
all-Pinhole batch, an all-EUCM batch and a mixed batch with Pinhole, EUCM, Fisheye624 and MEI members.

The torch composition is what a user writes from the reference's formulas: one batched expression for a batch of one class, a loop
over the images for the mixed batch (as the reference's BatchCamera does), then for the render the keep rules, the cell and one
scatter_reduce_(amin) per image.  A sample = `--calls` back-to-back calls between two device events, i.e. the time per call in a full
queue; median of `--reps` samples after warm-up.  Kernel times are NOT traced here: the figures include the launch and the Python of
each call.  Before anything is timed the two results are compared and the share of differing elements is reported.
Prints one JSON line.   python tools/bench_camera_project.py"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import _lib, cameras  # noqa: E402
from unidepth_amd.gtpoints import gt_points, prepare_camera  # noqa: E402
from unidepth_amd.reproject import project_camera, render_depth_camera  # noqa: E402

PINHOLE, EUCM, FISHEYE624, MEI = 1, 2, 5, 6


def batch_cameras(kind, B, hw):
    H, W = hw
    f, cx, cy = 0.8 * W, W / 2.0 + 1.3, H / 2.0 - 0.7
    make = {
        "pinhole": lambda i: cameras.Pinhole(params=torch.tensor([[f + i, f + 2.0 + i, cx, cy]])),
        "eucm": lambda i: cameras.EUCM(torch.tensor([[0.6 * f + i, 0.6 * f + 2.0 + i, cx, cy, 0.55, 1.1]])),
        "fisheye624": lambda i: cameras.Fisheye624(torch.tensor([[0.7 * f + i, 0.7 * f + 2.0, cx, cy, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 1e-3, -1e-3, 5e-4, 1e-4, -5e-4, 1e-4]])),
        "mei": lambda i: cameras.MEI(torch.tensor([[1.6 * f + i, 1.6 * f + 2.0, cx, cy, -0.1, 0.02, 1e-3, -1e-3, 0.9]])),
    }
    order = {"pinhole": ["pinhole"], "eucm": ["eucm"], "mixed": ["pinhole", "eucm", "fisheye624", "mei"]}[kind]
    return cameras.BatchCamera([make[order[i % len(order)]](float(i)) for i in range(B)])


def _tail(p, xr, yr, p0, p1, s):
    rd = xr * xr + yr * yr
    ud = xr + ((2.0 * xr * xr + rd) * p0 + 2.0 * xr * yr * p1)
    vd = yr + ((2.0 * yr * yr + rd) * p1 + 2.0 * xr * yr * p0)
    if s is not None:
        ud = ud + (s[0] * rd + s[1] * rd * rd)
        vd = vd + (s[2] * rd + s[3] * rd * rd)
    return ud * p[0] + p[2], vd * p[1] + p[3]


def torch_project(model, p, x, y, z):
    """the definitions of include/unidepth_hip.h (UdCameraProject) in torch; p: the parameter columns, each [B,1] (or scalars), x, y, z [B,N]"""
    if model == PINHOLE:
        zc = z.clamp(min=0.01)
        return (p[0] * x + p[2] * z) / zc, (p[1] * y + p[3] * z) / zc
    if model == EUCM:
        d = torch.sqrt(p[5] * (x * x + y * y) + z * z)
        den = (p[4] * d + (1.0 - p[4]) * z).clamp(min=1e-3)
        return p[0] * (x / den) + p[2], p[1] * (y / den) + p[3]
    if model == FISHEYE624:
        zz = torch.where(z.abs() < 1e-9, 1e-9 * torch.sign(z), z)
        a, b = x / zz, y / zz
        r = torch.sqrt(a * a + b * b)
        th = torch.atan(r)
        small = r < 1e-9
        dx, dy = torch.where(small, torch.ones_like(a), a / r), torch.where(small, torch.ones_like(b), b / r)
        t2 = th * th
        pw, s = th * t2, torch.zeros_like(th)
        for j in range(6):
            s = s + pw * p[4 + j]
            pw = pw * t2
        thk = th + s
        return _tail(p, thk * dx, thk * dy, p[10], p[11], p[12:16])
    n = torch.sqrt(x * x + y * y + z * z)
    den = z + p[8] * n
    a, b = x / den, y / den
    r2 = a * a + b * b
    fac = 1.0 + p[4] * r2 + p[5] * r2 * r2
    return _tail(p, a * fac, b * fac, p[6], p[7], None)


def torch_compose_project(pts, rows, models, hw):
    """pts [B,3,h,w] -> uv [B,2,h,w], inside [B,h,w]: one batched expression for a batch of one class, else image by image"""
    B, _, h, w = pts.shape
    H, W = hw

    def one(model, p, q):
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        u, v = torch_project(model, p, x, y, z)
        if model == PINHOLE:
            inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        else:
            inside = ~((u < 0) | (u > W) | (v < 0) | (v > H))
            if model == EUCM:
                inside &= ~(z < 0)
        return torch.stack([u, v], dim=1), inside

    if len(set(models)) == 1:
        return one(models[0], [rows[:, k].reshape(B, 1, 1) for k in range(16)], pts)
    parts = [one(models[b], [rows[b, k] for k in range(16)], pts[b:b + 1]) for b in range(B)]
    return torch.cat([a for a, _ in parts]), torch.cat([m for _, m in parts])


def torch_compose_render(pts, rows, models, hw):
    """the z-buffer of the projected points: [B,1,H,W], 0 where no point landed"""
    B = pts.shape[0]
    H, W = hw
    uv, _ = torch_compose_project(pts, rows, models, hw)
    x, y, z = (pts[:, k].reshape(B, -1) for k in range(3))
    u, v = uv[:, 0].reshape(B, -1), uv[:, 1].reshape(B, -1)
    fu, fv = torch.floor(u), torch.floor(v)
    ok = (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H) & (z > 0)
    mei = [b for b in range(B) if models[b] == MEI]
    if mei:
        n = torch.sqrt(x[mei] * x[mei] + y[mei] * y[mei] + z[mei] * z[mei])
        ok[mei] &= (z[mei] + rows[mei, 8:9] * n) > 0
    flat = (fu + fv * W).long()
    out = torch.full((B, H * W), float("inf"), device=pts.device)
    for b in range(B):
        out[b].scatter_reduce_(0, flat[b, ok[b]], z[b, ok[b]], "amin", include_self=True)
    return torch.where(torch.isinf(out), torch.zeros_like(out), out).view(B, 1, H, W)


def alternate_ms(fa, fb, calls, reps, warm=3):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, t in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / calls)
    return sorted(ta)[reps // 2], sorted(tb)[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, help="run the cases whose key contains this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_camera_project needs the GPU"
    B = 8
    res = {"op": "project_camera (1 launch) / render_depth_camera (3 launches; nearest, depth only) vs their torch compositions",
           "timing": "ms per call in a full queue (events around back-to-back calls, median); kernel times not traced",
           "reps": args.reps, "calls_per_sample": args.calls}
    for hw in ((518, 518), (480, 640)):
        H, W = hw
        g = torch.Generator().manual_seed(3)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        depth = ((3.0 + torch.sin(yy / 40.0) * torch.cos(xx / 55.0)).repeat(B, 1, 1) * (1.0 + 0.02 * torch.rand(B, H, W, generator=g)))[:, None].cuda()
        work = torch.empty(int(_lib.lib.ud_splat_work_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
        for kind in ("pinhole", "eucm", "mixed"):
            key = f"b{B}_{H}x{W}_{kind}"
            if args.only and args.only not in key:
                continue
            cam = batch_cameras(kind, B, hw)
            prepared = prepare_camera(cam, B, "cuda")
            rows, models = prepared.params, list(prepared.models)
            pts = gt_points(depth, prepared)
            uv, inside, _ = project_camera(pts, prepared)
            uv_t, inside_t = torch_compose_project(pts, rows, models, hw)
            view = render_depth_camera(pts, prepared, hw, workspace=work, return_count=True)
            view_t = torch_compose_render(pts, rows, models, hw)
            n = uv.numel()
            uv_differ = int(((uv - uv_t).abs() > 1e-3).sum())
            mask_differ = int((inside != inside_t).sum())
            px_differ = int((view.depth.view(torch.int32) != view_t.view(torch.int32)).sum())
            assert uv_differ <= 1e-3 * n and mask_differ <= 1e-3 * n and px_differ <= 1e-2 * view.depth.numel(), (key, uv_differ, mask_differ, px_differ)
            p_ms, p_torch = alternate_ms(lambda: project_camera(pts, prepared), lambda: torch_compose_project(pts, rows, models, hw), args.calls, args.reps)
            r_ms, r_torch = alternate_ms(lambda: render_depth_camera(pts, prepared, hw, workspace=work),
                                         lambda: torch_compose_render(pts, rows, models, hw), args.calls, args.reps)
            res[key] = {"points": B * H * W, "kept": int(view.count.sum()), "holes": int((view.depth == 0).sum()),
                        "project_camera_ms": round(p_ms, 4), "torch_project_ms": round(p_torch, 4), "project_speedup": round(p_torch / p_ms, 2),
                        "render_depth_camera_ms": round(r_ms, 4), "torch_render_ms": round(r_torch, 4), "render_speedup": round(r_torch / r_ms, 2),
                        "project_GBps": round(B * H * W * (12 + 8 + 1 + 4) / p_ms / 1e6, 1),
                        "uv_differing": uv_differ, "mask_differing": mask_differ, "render_differing_px": px_differ}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
