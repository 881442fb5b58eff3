"""Times remap.remap and remap.overlap_mask (ud_remap, ud_overlap_mask, csrc/remap.hip) on the GPU box: B = 8 at 518 x 518 and at
480 x 640, time per call in a full queue of calls (events around each call, median of a window; three windows after a warm-up,
alternating with the counterpart on the same GPU in the same process).

    depth_norm    C = 1 fp32 source with a source mask and coord_valid, normalised, with the validity returned
                  counterpart: coordinates normalised for F.grid_sample, grid_sample of src * mask and of the mask, their quotient, and
                  the validity arithmetic -- what a user writes without the kernel
    rgb_u8        C = 3 uint8 source to a uint8 result
                  counterpart: .float(), F.grid_sample, .round().clamp(0, 255).to(uint8)
    overlap_mask  counterpart: Camera.mask_overlap_projection's arithmetic in torch on the GPU
  each at two coordinate sets: the uv of a Fisheye624 -> Pinhole undistort (smooth: neighbouring points read neighbouring pixels), and a
  random permutation of the pixel grid (the uncoalesced worst case: every gather of a wave goes to another part of the image).

The times are events around Python calls on cache-warm buffers: a CALL RATE, close to the host's submission rate where the kernel is short.
Algorithmic bytes (every input and output once) divided by that time are printed as such: a lower bound of what the kernel moves per
second, not a measured bandwidth.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_remap.py --kernels-only
which only launches each workload 50 times; its rm_remap_kernel / rm_overlap_kernel rows are copied into the table by hand.
Prints one JSON line and writes the table to --out (default profiles/remap_bench.txt).
    python tools/bench_remap.py [--out PATH] [--kernels-only]"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import cameras  # noqa: E402
remap = importlib.import_module("unidepth_amd.remap")

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
    """one warm-up window of each, then WINDOWS windows of each, a b a b ...: ([ms of a], [ms of b])"""
    queue_ms(a, 20)
    queue_ms(b, 20)
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(queue_ms(a))
        tb.append(queue_ms(b))
    return ta, tb


def summary(ts):
    return round(sorted(ts)[len(ts) // 2], 4), [round(t, 4) for t in ts]


def torch_grid(uv, Hs, Ws):
    """our coordinates [B,2,H,W] as grid_sample's grid [B,H,W,2]: g = 2 u / Ws - 1 (align_corners=False)"""
    return torch.stack([uv[:, 0] * (2.0 / Ws) - 1.0, uv[:, 1] * (2.0 / Hs) - 1.0], dim=-1)


def torch_depth_norm(src, mask, uv, cv):
    Hs, Ws = src.shape[-2:]
    g = torch_grid(uv, Hs, Ws)
    m = mask.float()
    num = F.grid_sample(src * m, g, mode="bilinear", padding_mode="zeros", align_corners=False)
    den = F.grid_sample(m, g, mode="bilinear", padding_mode="zeros", align_corners=False)
    u, v = uv[:, 0:1], uv[:, 1:2]
    valid = cv & (u >= 0) & (u <= Ws) & (v >= 0) & (v <= Hs) & (den > 0)
    return torch.where(valid & (den > 0), num / den.clamp(min=1e-30), torch.zeros_like(num)), valid


def torch_rgb_u8(src, uv):
    Hs, Ws = src.shape[-2:]
    out = F.grid_sample(src.float(), torch_grid(uv, Hs, Ws), mode="bilinear", padding_mode="zeros", align_corners=False)
    return out.round().clamp(0, 255).to(torch.uint8)


def torch_overlap(projected):
    """Camera.mask_overlap_projection's arithmetic (unidepth/utils/camera.py:132-154) in torch"""
    B, _, H, W = projected.shape
    ident = torch.stack(torch.meshgrid(torch.arange(H, device=projected.device, dtype=torch.float32) + 0.5,
                                       torch.arange(W, device=projected.device, dtype=torch.float32) + 0.5, indexing="ij")[::-1])[None]
    flow = projected - ident
    s = 0.1 * flow + ident
    g = torch.stack([s[:, 0] / (W - 1) * 2 - 1, s[:, 1] / (H - 1) * 2 - 1], dim=-1)
    sampled = F.grid_sample(flow, g, mode="bilinear", align_corners=False, padding_mode="border")
    nf, ns = torch.norm(flow, dim=1, keepdim=True), torch.norm(sampled, dim=1, keepdim=True)
    return (0.9 * nf < ns) | (nf < 1)


def workloads(B, H, W):
    g = torch.Generator().manual_seed(0)
    depth = (0.5 + 40.0 * torch.rand(B, 1, H, W, generator=g)).cuda()
    hole = (torch.rand(B, 1, H, W, generator=g) >= 0.2).cuda()
    rgb = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8).cuda()
    fe = [0.4 * W, 0.4 * W + 1, W / 2 + 1, H / 2 - 1, 0.05, -0.01, 0.002, -0.0005, 1e-4, -1e-5, 1e-3, -1e-3, 0, 0, 0, 0]
    _, cv, uv = remap.undistort(depth, cameras.Fisheye624(torch.tensor(fe)), return_mask=True, return_uv=True)
    perm = torch.randperm(H * W, generator=g)
    gu = ((perm % W).float() + 0.5 + 0.3).view(1, 1, H, W)
    gv = ((perm // W).float() + 0.5 + 0.3).view(1, 1, H, W)
    scattered = torch.cat([gu, gv], 1).expand(B, 2, H, W).contiguous().cuda()
    every = torch.ones(B, 1, H, W, dtype=torch.bool, device="cuda")
    return depth, hole, rgb, {"undistort_uv": (uv.contiguous(), cv), "permuted_grid": (scattered, every)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch every workload 50 times and exit (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_remap.py needs a GPU"
    res = {"op": "remap / overlap_mask (maps sampled at arbitrary image coordinates)", "reps": REPS, "windows": WINDOWS}
    lines = ["tools/bench_remap.py on " + torch.cuda.get_device_name(0) + f": ms per call (a call rate), median of a window of {REPS} queued calls; "
             f"{WINDOWS} windows per arm after a warm-up, alternating with the torch composition; [..] = every window.",
             "GB/s = algorithmic bytes (every input and output once) per call time: a lower bound, not a measured bandwidth.", ""]
    B = 8
    for tag, (H, W) in {"b8_518x518": (518, 518), "b8_480x640": (480, 640)}.items():
        depth, hole, rgb, coords = workloads(B, H, W)
        n = B * H * W
        r = {}
        lines.append(f"{tag}  (B = {B}, {H * W} points per image)")
        for cname, (uv, cv) in coords.items():
            a1 = lambda: remap.remap(depth, uv, src_mask=hole, coord_valid=cv, normalize=True, return_mask=True)       # noqa: E731
            b1 = lambda: torch_depth_norm(depth, hole, uv, cv)                                                        # noqa: E731
            a2 = lambda: remap.remap(rgb, uv)                                                                         # noqa: E731
            b2 = lambda: torch_rgb_u8(rgb, uv)                                                                        # noqa: E731
            a3 = lambda: remap.overlap_mask(uv)                                                                       # noqa: E731
            b3 = lambda: torch_overlap(uv)                                                                            # noqa: E731
            if args.kernels_only:
                for fn in (a1, a2, a3):
                    for _ in range(50):
                        fn()
                torch.cuda.synchronize()
                continue
            o, v = a1()
            to, tv = b1()
            # where the live taps weigh less than 1e-2 the quotient amplifies the rounding of grid_sample's normalised coordinates: left out
            den = F.grid_sample(hole.float(), torch_grid(uv, H, W), mode="bilinear", padding_mode="zeros", align_corners=False)
            both = v & tv & (den > 1e-2)
            r[f"{cname}_depth_norm_max_rel_diff_vs_torch"] = float(((o - to).abs() / to.abs().clamp(min=1))[both].max())
            r[f"{cname}_depth_norm_valid_differ"] = int((v != tv).sum())
            r[f"{cname}_rgb_u8_max_abs_diff_vs_torch"] = int((a2().int() - b2().int()).abs().max())
            r[f"{cname}_overlap_differ"] = int((a3() != b3()).sum())
            nbytes = {"depth_norm": n * (4 + 1 + 8 + 1 + 4 + 1), "rgb_u8": n * (3 + 8 + 3), "overlap_mask": n * (8 + 1)}
            for wname, a, b in (("depth_norm", a1, b1), ("rgb_u8", a2, b2), ("overlap_mask", a3, b3)):
                ta, tb = alternate(a, b)
                (r[f"{cname}_{wname}_ms"], r[f"{cname}_{wname}_runs_ms"]), (r[f"{cname}_{wname}_torch_ms"], r[f"{cname}_{wname}_torch_runs_ms"]) = summary(ta), summary(tb)
                gbs = nbytes[wname] / (summary(ta)[0] * 1e-3) / 1e9
                r[f"{cname}_{wname}_algorithmic_GBps_at_call_rate"] = round(gbs, 1)
                lines.append(f"  {cname:13s} {wname:12s} kernel path {summary(ta)[0]:.4f} {summary(ta)[1]}  torch {summary(tb)[0]:.4f} {summary(tb)[1]}  "
                             f"{nbytes[wname] / 1e6:.1f} MB algorithmic, {gbs:.0f} GB/s at the call rate")
            lines.append(f"  {cname:13s} agreement: depth_norm max rel diff (weight sum > 1e-2) {r[f'{cname}_depth_norm_max_rel_diff_vs_torch']:.2e} "
                         f"({r[f'{cname}_depth_norm_valid_differ']} validity differ), rgb_u8 max abs diff {r[f'{cname}_rgb_u8_max_abs_diff_vs_torch']}, "
                         f"overlap_mask {r[f'{cname}_overlap_differ']} of {n} pixels differ")
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
