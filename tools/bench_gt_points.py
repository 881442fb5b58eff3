"""Times gtpoints.gt_points (ud_reconstruct, csrc/reconstruct.hip) on the GPU box: B = 8 at 480 x 640 and at 375 x 1242, time per
call in a full queue of calls (events around each call, median), for an all-Pinhole batch, an all-EUCM batch and a mixed batch with
two OPENCV and two Fisheye624 members (plus Pinhole, EUCM, Spherical, MEI).  The closed-form batches alternate on the same GPU and
inputs with a torch composition of the same definitions, what a user writes without gt_points; the iterative solvers have no torch
composition here (nobody writes those twice), so the mixed batch stands alone.  Camera rows are uploaded once (prepare_camera), as a
validation loop over one dataset does.  The times are events around Python calls on cache-warm buffers: a call rate, which at these sizes
is close to the host's submission rate; no kernel trace is taken and no bandwidth is derived.  Prints one JSON line.
    python tools/bench_gt_points.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import cameras, gtpoints  # noqa: E402


def queue_ms(fn, reps=20):
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


def grid(H, W):
    u = (torch.arange(W, device="cuda", dtype=torch.float32) + 0.5).view(1, 1, W)
    v = (torch.arange(H, device="cuda", dtype=torch.float32) + 0.5).view(1, H, 1)
    return u, v


def torch_pinhole(depth, p):
    """K^-1 [u, v, 1] * max(depth, 0) in torch: p [B,4] on the device"""
    B, _, H, W = depth.shape
    u, v = grid(H, W)
    fx, fy, cx, cy = (p[:, i].view(B, 1, 1) for i in range(4))
    x = ((u - cx) / fx).expand(B, H, W)
    y = ((v - cy) / fy).expand(B, H, W)
    return torch.stack([x, y, torch.ones_like(x)], 1) * depth.clamp(min=0.0)


def torch_eucm(depth, p):
    """the EUCM row of the definition table in torch: p [B,6] on the device"""
    B, _, H, W = depth.shape
    u, v = grid(H, W)
    fx, fy, cx, cy, al, be = (p[:, i].view(B, 1, 1) for i in range(6))
    mx, my = ((u - cx) / fx).expand(B, H, W), ((v - cy) / fy).expand(B, H, W)
    r2 = mx * mx + my * my
    mz = (1 - be * al * al * r2) / (al * torch.sqrt((1 - (2 * al - 1) * be * r2).clamp(min=1e-5)) + (1 - al))
    c = 1 / torch.sqrt(mx * mx + my * my + mz * mz + 1e-5)
    r = torch.stack([c * mx, c * my, (c * mz).clamp(min=1e-3)], 1)
    return r / r[:, 2:].clamp(min=1e-4) * depth.clamp(min=1e-4)


def main():
    res = {"op": "gt_points (Camera.reconstruct of a batch, one camera model per image)"}
    B = 8
    for tag, (H, W) in {"b8_480x640": (480, 640), "b8_375x1242": (375, 1242)}.items():
        g = torch.Generator().manual_seed(0)
        depth = (0.5 + 40.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
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
        r = {}
        for name, cam in cams.items():
            hip = lambda: gtpoints.gt_points(depth, cam)                       # noqa: E731
            out = hip()
            a, b = [], []
            if name in torch_fns:
                fn, p = torch_fns[name]
                comp = lambda: fn(depth, p)                                    # noqa: E731
                ref = comp()
                r[name + "_max_abs_diff_vs_torch"] = float((out - ref).abs().max())
            for _ in range(3):                                                 # alternate the two on the same GPU
                a.append(queue_ms(hip))
                if name in torch_fns:
                    b.append(queue_ms(comp))
            r[name + "_ms"] = round(sorted(a)[1], 4)
            r[name + "_runs_ms"] = [round(x, 4) for x in a]
            if b:
                r[name + "_torch_ms"] = round(sorted(b)[1], 4)
                r[name + "_torch_runs_ms"] = [round(x, 4) for x in b]
                r[name + "_speedup"] = round(r[name + "_torch_ms"] / r[name + "_ms"], 2)
        res[tag] = r
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
