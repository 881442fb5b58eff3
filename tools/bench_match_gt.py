"""Times the fused validation matching (one ud_match_gt, csrc/matchgt.hip: depth, points = rays * radius, confidence and the intrinsics of a
batch, per-image paddings) next to the torch composition a user writes without it -- the reference's per-image loop restated: the
product rays * radius at network resolution, then for every image and every map slice, F.interpolate, F.pad, and torch.cat per map,
plus the intrinsics loop -- on the same GPU, same process, alternating runs.  B = 8, 518 x 518 -> 480 x 640 and -> 375 x 1242, four
maps (depth, points, confidence, intrinsics).  Device events after warm-up, median of the timed runs; the two results are compared
first (the composition associates the four products differently: agreement to a few ulp, not bit equality).  The bytes are the
algorithm's: every source read once (rays, radius, confidence), every destination written once.  Prints one JSON line.
    python tools/bench_match_gt.py"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import matching  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E datasheet


def inputs(B, Hn, Wn, seed=0):
    g = torch.Generator().manual_seed(seed)
    rays = F.normalize(torch.randn(B, 3, Hn, Wn, generator=g), dim=1)
    radius = 1.0 + 6.0 * torch.rand(B, 1, Hn, Wn, generator=g)
    conf = torch.rand(B, 1, Hn, Wn, generator=g)
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 400.0, 410.0, Wn / 2.0, Hn / 2.0
    # a different padding per image, multiples of the patch size as the datasets produce them
    pads = [(14 * (b % 3), 14 * ((b + 1) % 2), 14 * (b % 2), 14 * ((b + 2) % 3)) for b in range(B)]
    return rays.cuda(), radius.cuda(), conf.cuda(), K.cuda(), pads


def fused(rays, radius, conf, K, pads, H2, W2):
    B, _, Hn, Wn = rays.shape
    dev = rays.device
    out = {"depth": torch.empty(B, 1, H2, W2, device=dev), "points": torch.empty(B, 3, H2, W2, device=dev),
           "confidence": torch.empty(B, 1, H2, W2, device=dev), "intrinsics": torch.empty(B, 3, 3, device=dev)}
    d1, _ = matching.upload_paddings(pads, None, dev)
    npx = Hn * Wn
    matching.launch([dict(src=rays, mul=radius, dst=out["points"], C=3, src_batch_stride=3 * npx),
                     dict(src=rays.data_ptr() + 2 * npx * 4, mul=radius, dst=out["depth"], C=1, src_batch_stride=3 * npx),
                     dict(src=conf, dst=out["confidence"], C=1, src_batch_stride=npx)], B, Hn, Wn, H2, W2, d1, None, K, out["intrinsics"])
    return out


def torch_compose(rays, radius, conf, K, pads, H2, W2):
    B, _, Hn, Wn = rays.shape
    points = rays * radius

    def match(t):
        outs = []
        for b in range(B):
            l, r, tp, bt = pads[b]
            outs.append(F.pad(F.interpolate(t[b:b + 1, :, tp:Hn - bt, l:Wn - r], size=(H2, W2), mode="bilinear"), (0, 0, 0, 0)))
        return torch.cat(outs)

    Kn = K.clone()
    for b in range(B):
        l, r, tp, bt = pads[b]
        sx, sy = W2 / (Wn - l - r), H2 / (Hn - tp - bt)
        Kn[b, 0, 0] *= sx
        Kn[b, 1, 1] *= sy
        Kn[b, 0, 2] = (K[b, 0, 2] - l) * sx
        Kn[b, 1, 2] = (K[b, 1, 2] - tp) * sy
    return {"depth": match(points[:, 2:]), "points": match(points), "confidence": match(conf), "intrinsics": Kn}


def alternate_ms(fa, fb, reps=21, warm=3):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, t in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return sorted(ta)[reps // 2], sorted(tb)[reps // 2]


def main():
    assert torch.cuda.is_available(), "bench_match_gt needs the GPU"
    B, Hn, Wn = 8, 518, 518
    res = {"op": "forward_test matching: depth + points (rays * radius) + confidence + intrinsics, per-image paddings", "launches": 1,
           "reps": 21}
    rays, radius, conf, K, pads = inputs(B, Hn, Wn)
    for H2, W2 in ((480, 640), (375, 1242)):
        def ours():
            return fused(rays, radius, conf, K, pads, H2, W2)

        def theirs():
            return torch_compose(rays, radius, conf, K, pads, H2, W2)

        a, b = ours(), theirs()
        torch.cuda.synchronize()
        for k in a:
            err = ((a[k] - b[k]).abs() / b[k].abs().clamp_min(1.0)).max().item()
            assert err < 2e-5, (k, err)
        ms, ms_torch = alternate_ms(ours, theirs)
        nbytes = 4 * B * (5 * Hn * Wn + 5 * H2 * W2) + 2 * 36 * B
        res[f"b{B}_{Hn}x{Wn}_to_{H2}x{W2}"] = {
            "match_gt_ms": round(ms, 4), "torch_compose_ms": round(ms_torch, 4), "speedup": round(ms_torch / ms, 2),
            "MB_moved": round(nbytes / 1e6, 1), "GBps": round(nbytes / ms / 1e6, 1), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
