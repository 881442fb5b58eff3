"""Times reproject.render_depth (ud_splat, csrc/splat.hip) next to the torch composition a user writes without it, on the same GPU, same
process, alternating: B = 8 clouds of 518 x 518 points into 518 x 518 and into 480 x 640 images, from planar points [B,3,h,w] and from a
packed PointCloud, in both modes.  The torch composition is project_points' recipe for the mean (matmul with K^T, divide, truncate, mask,
one scatter_add_ of depths and one of ones per image, divide) and the same projection followed by scatter_reduce_(amin) per image for
the nearest surface; for the packed cloud it gets the per-image row ranges as host integers for free (reading them is a synchronisation
a user pays and render_depth does not).

A sample = `--calls` back-to-back calls between two device events; median of `--reps` samples after warm-up, per call.  Before anything
is timed the two results are compared: the share of pixels where they differ is reported (torch's matmul sums in its own order, so a
point next to a cell edge can land on the other side; ud_splat's arithmetic is fixed by include/unidepth_hip.h).  The bytes are the
algorithm's: 12 B per point read, one 8-B atomic per kept point (+ 4 B in mean mode), and per destination pixel 8 (12) B filled, 8 (12) B
read back and 4 B written.  Prints one JSON line.   python tools/bench_render_depth.py"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import _lib  # noqa: E402
from unidepth_amd.pointcloud import PointCloud  # noqa: E402
from unidepth_amd.reproject import render_depth  # noqa: E402

SRC = (518, 518)


def inputs(B, dst, seed=0):
    """A smooth depth map per image unprojected at its pixel centres (u + 0.5) with the source intrinsics, and destination intrinsics that
    zoom by 1.07 and shift the principal point: several points on some pixels, none on others, a margin that leaves the image."""
    h, w = SRC
    H, W = dst
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64) + 0.5, torch.arange(w, dtype=torch.float64) + 0.5, indexing="ij")
    z = (3.0 + torch.sin(yy / 40.0) * torch.cos(xx / 55.0)).repeat(B, 1, 1) * (1.0 + 0.02 * torch.rand(B, h, w, generator=g).double())
    f, cx, cy = 0.9 * w, w / 2.0, h / 2.0
    pts = torch.stack([(xx - cx) * z / f, (yy - cy) * z / f, z], dim=1).float()
    K = torch.tensor([[1.07 * f * W / w, 0.0, W / 2.0 + 3.3], [0.0, 1.07 * f * W / w, H / 2.0 - 2.1], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    return pts.cuda(), K.cuda()


def torch_compose(rows, K, dst, mode, ranges=None):
    """rows [B,N,3] (or packed [n,3] with per-image host ranges) -> [B,1,H,W]."""
    H, W = dst
    if ranges is not None:
        rows = torch.stack([rows[a:b] for a, b in ranges])             # the bench's images have equal counts
    B = rows.shape[0]
    uvw = torch.matmul(rows, K.transpose(1, 2))
    uv = (uvw[..., :2] / uvw[..., 2:]).int()
    z = rows[..., 2]
    ok = (uv[..., 0] >= 0) & (uv[..., 0] < W) & (uv[..., 1] >= 0) & (uv[..., 1] < H)
    if mode == "nearest":
        ok &= z > 0
    flat = (uv[..., 0] + uv[..., 1] * W).long()
    out = torch.zeros(B, H * W, device=rows.device)
    if mode == "mean":
        cnt = torch.zeros(B, H * W, device=rows.device)
        for b in range(B):
            i, zb = flat[b, ok[b]], z[b, ok[b]]
            out[b].scatter_add_(0, i, zb)
            cnt[b].scatter_add_(0, i, torch.ones_like(zb))
        out = out / cnt.clamp(min=1.0)
    else:
        for b in range(B):
            out[b].scatter_reduce_(0, flat[b, ok[b]], z[b, ok[b]], "amin", include_self=False)
    return out.view(B, 1, H, W)


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
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--only", default=None, help="run the cases whose key contains this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render_depth needs the GPU"
    B = 8
    res = {"op": "render_depth (depth only; rounding trunc, pixel_offset 0)", "launches": 3, "reps": args.reps, "calls_per_sample": args.calls}
    for dst in ((518, 518), (480, 640)):
        pts, K = inputs(B, dst)
        n = SRC[0] * SRC[1]
        rows = pts.reshape(B, 3, n).permute(0, 2, 1).contiguous()
        cloud = PointCloud(rows.reshape(-1, 3), None, None, torch.full((B,), n, dtype=torch.int64).cuda(), torch.arange(B + 1, dtype=torch.int64).cuda() * n)
        ranges = [(b * n, (b + 1) * n) for b in range(B)]
        work = torch.empty(int(_lib.lib.ud_splat_work_bytes(B, *dst)), dtype=torch.uint8, device="cuda")
        for source in ("planar", "packed"):
            for mode in ("nearest", "mean"):
                key = f"b{B}_{SRC[0]}x{SRC[1]}_to_{dst[0]}x{dst[1]}_{source}_{mode}"
                if args.only and args.only not in key:
                    continue

                def ours():
                    return render_depth(pts if source == "planar" else cloud, K, dst, mode=mode, rounding="trunc", workspace=work, return_count=True).depth

                def ours_timed():
                    return render_depth(pts if source == "planar" else cloud, K, dst, mode=mode, rounding="trunc", workspace=work).depth

                def theirs():
                    if source == "planar":                                 # the [B,N,3] rows the recipe wants are part of its cost
                        return torch_compose(pts.reshape(B, 3, n).permute(0, 2, 1), K, dst, mode)
                    return torch_compose(cloud.xyz, K, dst, mode, ranges)

                a, b = ours(), theirs()
                kept = int(render_depth(pts, K, dst, mode=mode, rounding="trunc", workspace=work, return_count=True).count.sum())
                if mode == "nearest":
                    differ = int((a.view(torch.int32) != b.view(torch.int32)).sum())
                else:
                    differ = int(((a - b).abs() > 2.0 ** -20 * b.abs().clamp(min=1.0)).sum())
                px = B * dst[0] * dst[1]
                assert differ <= 1e-2 * px, (key, differ)              # a gross disagreement is a bug in one of the two; the count is reported
                ms, ms_torch = alternate_ms(ours_timed, theirs, args.calls, args.reps)
                word = 12 if mode == "mean" else 8
                nbytes = B * n * 12 + kept * word + px * (2 * word + 4)
                res[key] = {"points": B * n, "kept": kept, "holes": int((a == 0).sum()), "render_depth_ms": round(ms, 4), "torch_compose_ms": round(ms_torch, 4),
                            "speedup": round(ms_torch / ms, 2), "MB_per_call": round(nbytes / 1e6, 1), "call_rate_GBps": round(nbytes / ms / 1e6, 1),
                            "torch_compose_differing_px": differ}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
