"""Times the fused validation-input step (one ud_resize_aa, csrc/testprep.hip: window, antialiased bicubic resize, byte rounding, /255,
normalise, validity mask, intrinsics) next to the torch composition a user writes without it -- per plane slice, F.pad,
F.interpolate(antialias=True), round, clamp, /255, normalise, plus the nearest mask and the camera arithmetic
(tools/make_golden_testprep.py torch_composition) -- on the same GPU, same process, alternating samples.
    B = 8 uint8 images 480 x 640 and 375 x 1242 -> the network shape test_geometry gives under the released ViT-L shape_constraints,
    and original_image (bilinear, antialiased) from that shape back to the source size.
A sample is CALLS back-to-back calls between two device events (the time per call at which a full queue drains, launch latency hidden),
median of the samples after warm-up; the two results are compared first.  The bytes are the algorithm's: every source byte of the
window that exists read once, every destination written once.  Prints one JSON line.
    python tools/bench_testprep.py                 the timing
    python tools/bench_testprep.py --calls-only    only the fused calls, for one kernel trace of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python tools/bench_testprep.py --calls-only
    python tools/bench_testprep.py --kernel-trace <dir>/.../t_kernel_trace.csv     adds the traced kernel times (median per shape, the
        20 dispatches of each shape in launch order) and the algorithm's bytes over them against the HBM peak to the JSON line"""
import csv
import importlib.util
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import testprep  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_testprep", os.path.join(ROOT, "tools", "make_golden_testprep.py"))
tp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tp)

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E datasheet
CALLS, SAMPLES, WARM = 50, 11, 2
KERNEL = "ud_resize_aa_kernel"
CONS = tp.CONSTRAINTS["v2"]
SHAPES = ((480, 640), (375, 1242))


def inputs(B, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.9 * w, 0.9 * w, w / 2.0, h / 2.0
    return img.cuda(), K.cuda()


def fused(img, K):
    return testprep.prepare_test_batch(img, camera=K, image_shape=tp.IMAGE_SHAPE, shape_constraints=CONS)[0]


def torch_compose(img, K, geo):
    (Hn, Wn), win = geo.shape, geo.window
    image = tp.torch_composition(img, win, (Hn, Wn), "bicubic", out="norm")
    ones = torch.ones(img.shape[0], 1, *img.shape[-2:], device=img.device)
    top, left, height, width = win
    m = F.pad(ones, (max(-left, 0), max(left + width - img.shape[-1], 0), max(-top, 0), max(top + height - img.shape[-2], 0)))
    mask = F.interpolate(m, size=(Hn, Wn), mode="nearest").to(torch.uint8)
    Kn = K.clone()
    Kn[:, 0, 2] -= left
    Kn[:, 1, 2] -= top
    Kn[:, :2, :] *= geo.zoom
    return {"image": image, "validity_mask": mask, "camera": Kn}


def back_fused(net, gt, metas):
    return testprep.original_image({"data": {"image": net, "depth": gt}, "img_metas": metas})[0]["data"]["image"]


def back_compose(net, hw, pads):
    left, top, right, bottom = pads
    full = F.interpolate(net, size=(hw[0] + top + bottom, hw[1] + left + right), mode="bilinear", antialias=True, align_corners=False)
    return full[..., top:top + hw[0], left:left + hw[1]].contiguous()


def queue_ms(fa, fb):
    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS
    for _ in range(WARM):
        sample(fa)
        sample(fb)
    ta, tb = [], []
    for _ in range(SAMPLES):
        ta.append(sample(fa))
        tb.append(sample(fb))
    return sorted(ta)[SAMPLES // 2], sorted(tb)[SAMPLES // 2]


def window_bytes(B, C, hw, win):
    top, left, height, width = win
    rows = max(min(top + height, hw[0]) - max(top, 0), 0)
    cols = max(min(left + width, hw[1]) - max(left, 0), 0)
    return B * C * rows * cols


def cases():
    B = 8
    for hw in SHAPES:
        img, K = inputs(B, *hw)
        geo = testprep.test_geometry(hw, tp.IMAGE_SHAPE, CONS)
        yield B, hw, img, K, geo


def prepare_bytes(B, hw, geo):
    return window_bytes(B, 3, hw, geo.window) + B * geo.shape[0] * geo.shape[1] * (3 * 4 + 1) + 2 * 36 * B


def kernel_times(path):
    """median duration per shape of the ud_resize_aa dispatches of a --calls-only run (launch order: 20 per shape)"""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if KERNEL in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    n = len(dur) // len(SHAPES)
    out = {"dispatches": len(dur)}
    for i, (hw, c) in enumerate(zip(SHAPES, cases())):
        d = sorted(dur[i * n:(i + 1) * n])
        if d:
            us = d[len(d) // 2]
            nbytes = prepare_bytes(c[0], hw, c[4])
            out["%dx%d" % hw] = {"kernel_us": round(us, 2), "GBps": round(nbytes / us / 1e3, 1), "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
    return out


def main():
    assert torch.cuda.is_available(), "bench_testprep needs the GPU"
    if "--calls-only" in sys.argv:
        for B, hw, img, K, geo in cases():
            for _ in range(20):
                fused(img, K)
        torch.cuda.synchronize()
        return
    res = {"op": "prepare_test_batch: window + antialiased bicubic + byte rounding + /255 + normalise + mask + intrinsics; original_image back",
           "launches": 1, "samples": SAMPLES, "calls_per_sample": CALLS}
    for B, hw, img, K, geo in cases():
        (Hn, Wn), win = geo.shape, geo.window
        a, b = fused(img, K), torch_compose(img, K, geo)
        torch.cuda.synchronize()
        # the library's own fp32 rounding can move a value across a half-integer: bytes differ by one level in a few pixels per million
        step = (1.0 / 255.0) / min(tp.STD)
        diff = (a["image"] - b["image"]).abs()
        assert float(diff.max()) <= 1.01 * step and float((diff > 1e-4).float().mean()) < 0.02, (float(diff.max()), float((diff > 1e-4).float().mean()))
        assert torch.equal(a["validity_mask"], b["validity_mask"]) and float((a["camera"] - b["camera"]).abs().max()) < 1e-3
        ms, ms_torch = queue_ms(lambda: fused(img, K), lambda: torch_compose(img, K, geo))
        nbytes = prepare_bytes(B, hw, geo)
        key = f"b{B}_{hw[0]}x{hw[1]}_to_{Hn}x{Wn}"
        res[key] = {"prepare_ms": round(ms, 4), "torch_compose_ms": round(ms_torch, 4), "speedup": round(ms_torch / ms, 2),
                    "differing_bytes_share": round(float((diff > 1e-4).float().mean()), 6),
                    "MB_per_call": round(nbytes / 1e6, 2), "call_rate_GBps": round(nbytes / ms / 1e6, 1)}
        net = a["image"]
        metas = [{"paddings": list(geo.paddings)}] * B
        gt = torch.empty(B, 1, *hw, device="cuda")
        x, y = back_fused(net, gt, metas), back_compose(net, hw, geo.paddings)
        torch.cuda.synchronize()
        assert float((x - y).abs().max()) < 1e-4, float((x - y).abs().max())
        ms, ms_torch = queue_ms(lambda: back_fused(net, gt, metas), lambda: back_compose(net, hw, geo.paddings))
        nbytes = 4 * B * 3 * (Hn * Wn + hw[0] * hw[1])
        res[f"b{B}_{Hn}x{Wn}_back_to_{hw[0]}x{hw[1]}"] = {
            "original_image_ms": round(ms, 4), "torch_compose_ms": round(ms_torch, 4), "speedup": round(ms_torch / ms, 2),
            "MB_per_call": round(nbytes / 1e6, 2), "call_rate_GBps": round(nbytes / ms / 1e6, 1)}
    if "--kernel-trace" in sys.argv:
        res["kernel_trace"] = kernel_times(sys.argv[sys.argv.index("--kernel-trace") + 1])
    res["hbm_peak_GBps"] = HBM_PEAK / 1e9
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
