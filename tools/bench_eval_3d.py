"""Times eval_ops.eval_3d_batch (ud_eval_3d, csrc/eval3d.hip) on the GPU box, alternating on the same GPU and inputs with the unchanged
eval_ops.eval_3d loop (host synchronisations, three F.interpolate, four ud_knn_points searches and ~6 T tiny launches per image).
Two cases: B = 8 at 480 x 640 and B = 8 at 518 x 518, ~70 % valid, T = 100 (thresholds_3d(0.01, 10.0)).  eval_3d_batch is timed per
call in a full queue of calls (events around each call, median); the loop synchronises the host, so it is timed by the wall clock.
The kernel times of the new launches come from a torch.profiler trace of the same queue.  Prints one JSON line.
    python tools/bench_eval_3d.py"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import eval_ops  # noqa: E402

KERNELS = ("e3_count_kernel", "e3_size_kernel", "e3_flag_kernel", "e3_scan_kernel", "e3_pack_kernel", "e3_knn_kernel", "e3_partial_kernel",
           "e3_final_kernel")


def inputs(B, H, W, keep=0.7, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = 1.0 + 4.0 * torch.rand(B, 1, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(-0.6, 0.6, H), torch.linspace(-0.8, 0.8, W), indexing="ij")
    gts = torch.cat([xx[None, None] * z, yy[None, None] * z, z], 1)
    preds = gts * (1.0 + 0.03 * torch.randn(B, 3, H, W, generator=g)) + 0.01 * torch.randn(B, 3, H, W, generator=g)
    masks = torch.rand(B, 1, H, W, generator=g) < keep
    return gts.cuda(), preds.cuda(), masks.cuda()


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


def wall_ms(fn, reps=3):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[reps // 2]


def kernel_us(fn, reps=10):
    """mean device time per launch of every ud_eval_3d kernel over `reps` queued calls (torch.profiler)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        for k in KERNELS:
            if k in e.key:
                total = getattr(e, "device_time_total", None)
                if total is None:
                    total = e.cuda_time_total
                out[k] = round(total / max(e.count, 1), 2)
    return out


def main():
    res = {"op": "eval_3d_batch (MSE_3d, chamfer, F1 per image; T = 100)"}
    for tag, (B, H, W) in {"b8_480x640_70pct": (8, 480, 640), "b8_518x518_70pct": (8, 518, 518)}.items():
        gts, preds, masks = inputs(B, H, W)
        th = eval_ops.thresholds_3d(0.01, 10.0, device="cuda")
        batch = lambda: eval_ops.eval_3d_batch(gts, preds, masks, th)          # noqa: E731
        loop = lambda: eval_ops.eval_3d(gts, preds, masks, th)                 # noqa: E731
        batch(), loop()
        a, b = [], []
        for _ in range(3):                                                     # alternate the two on the same GPU
            a.append(queue_ms(batch))
            b.append(wall_ms(loop))
        r = {"eval_3d_batch_ms": round(sorted(a)[1], 4), "eval_3d_loop_ms": round(sorted(b)[1], 2), "eval_3d_batch_runs_ms": [round(v, 4) for v in a],
             "eval_3d_loop_runs_ms": [round(v, 2) for v in b], "launches": len(KERNELS)}
        r["speedup"] = round(r["eval_3d_loop_ms"] / r["eval_3d_batch_ms"], 1)
        out = batch()
        r["size"] = out["size"].tolist()
        r["points_per_image"] = out["count"].tolist()
        try:
            ku = kernel_us(batch)
            r["kernel_us"] = ku
            if ku:
                r["kernel_sum_us"] = round(sum(ku.values()), 1)
                r["knn_share"] = round(ku.get("e3_knn_kernel", 0.0) / max(sum(ku.values()), 1e-9), 3)
        except Exception as e:                                                 # the trace is optional: say why it is missing
            r["kernel_us"] = f"not measured ({type(e).__name__}: {e})"
        res[tag] = r
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
