"""Times pointcloud.pack_points (ud_pointcloud_pack, csrc/pointcloud.hip) with `capacity` given, next to the torch composition a user
writes without it (mask arithmetic, nonzero, index_select of the point and colour rows) on the same GPU, same process, alternating runs.
B = 8 at 518 x 518 and at 480 x 640; 100 %, 85 % and 10 % of the pixels valid; with and without the edge (flying-pixel) filter.
Device events after warm-up, median of the timed runs; both results are compared bit for bit before anything is timed.  The bytes are the
algorithm's: every input map once in the flag pass (the edge filter's neighbours are cache hits), one bit per pixel written and read
back, and the payload of the valid pixels read and written once.  Prints one JSON line.   python tools/bench_pointcloud.py"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unidepth_amd import _lib, pointcloud  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E datasheet
RTOL = 0.05


def inputs(B, H, W, frac, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = (3.0 + torch.sin(yy / 40.0) * torch.cos(xx / 55.0)).repeat(B, 1, 1, 1) * (1.0 + 0.002 * torch.randn(B, 1, H, W, generator=g))
    z = torch.where(torch.rand(B, 1, H, W, generator=g) < 0.02, z * 1.4, z)                 # flying pixels for the edge filter
    pts = torch.cat([torch.randn(B, 2, H, W, generator=g) * z, z], dim=1).float()
    image = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    mask = torch.rand(B, 1, H, W, generator=g) < frac if frac < 1.0 else torch.ones(B, 1, H, W, dtype=torch.bool)
    return pts.cuda(), z.float().cuda(), image.cuda(), mask.cuda()


def torch_compose(pts, depth, image, mask, edge):
    """What a user writes today: a validity map, nonzero (a host synchronisation), and row gathers."""
    B, _, H, W = pts.shape
    v = mask[:, 0] & torch.isfinite(pts).all(dim=1)
    if edge:
        d = depth[:, 0]

        def ok(a, n):
            return (a - n).abs() <= RTOL * torch.minimum(a, n)

        v = v.clone()
        v[:, :, 1:] &= ok(d[:, :, 1:], d[:, :, :-1])
        v[:, :, :-1] &= ok(d[:, :, :-1], d[:, :, 1:])
        v[:, 1:, :] &= ok(d[:, 1:, :], d[:, :-1, :])
        v[:, :-1, :] &= ok(d[:, :-1, :], d[:, 1:, :])
    idx = v.reshape(-1).nonzero().squeeze(1)
    xyz = pts.permute(0, 2, 3, 1).reshape(-1, 3).index_select(0, idx)
    rgb = image.permute(0, 2, 3, 1).reshape(-1, 3).index_select(0, idx)
    return xyz, rgb, v.reshape(B, -1).sum(dim=1)


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
    assert torch.cuda.is_available(), "bench_pointcloud needs the GPU"
    res = {"op": "pack_points (xyz + u8 rgb rows, capacity given)", "launches": 4, "reps": 21}
    for B, H, W in ((8, 518, 518), (8, 480, 640)):
        for frac in (1.0, 0.85, 0.10):
            pts, depth, image, mask = inputs(B, H, W, frac)
            work = torch.empty(int(_lib.lib.ud_pointcloud_work_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
            for edge in (False, True):
                def ours():
                    return pointcloud.pack_points(pts, depth=depth, image=image, mask=mask, edge_rtol=RTOL if edge else None,
                                                  capacity=B * H * W, workspace=work)

                def theirs():
                    return torch_compose(pts, depth, image, mask, edge)

                pc, (xyz, rgb, cnt) = ours(), theirs()
                n = int(pc.offsets[-1])
                assert n == xyz.shape[0] and torch.equal(pc.counts, cnt), (n, xyz.shape)
                assert torch.equal(pc.xyz[:n].view(torch.int32), xyz.view(torch.int32)) and torch.equal(pc.rgb[:n], rgb)
                ms, ms_torch = alternate_ms(ours, theirs)
                npx = B * H * W
                nbytes = npx * (1 + 12 + 4) + 2 * npx // 8 + n * 2 * (12 + 3)
                res[f"b{B}_{H}x{W}_valid{int(frac * 100)}{'_edge' if edge else ''}"] = {
                    "rows": n, "pack_points_ms": round(ms, 4), "torch_compose_ms": round(ms_torch, 4), "speedup": round(ms_torch / ms, 2),
                    "MB_moved": round(nbytes / 1e6, 1), "GBps": round(nbytes / ms / 1e6, 1), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
