"""Times tsdfmesh.tsdf_mesh (ud_tsdf_mesh, csrc/tsdf_mesh.hip) against its two yardsticks on the GPU box: tsdf_mesh_composition, the same
definition in vectorised torch, and tsdf.tsdf_points on the same volume (the packer the mesh is built from: one compaction over slots where
the mesh runs one over cells and one over slots).  The volumes are tools/bench_tsdf.py's scene -- a plane with a block, 8 mixed-model
views of 480 x 640 with weights and colours fused by tsdf_integrate -- at 128^3 and 256^3, B = 1.

    counted          tsdf_mesh(volume): count, one read-back of both totals, allocate, pack (what tsdf_points' timed form also does)
    given            tsdf_mesh(volume, vert_capacity=, face_capacity=): one call, no host synchronisation
    +normals         the same with return_normals=True

Before timing, every output of the fused call is compared with the composition's bit for bit at the timed size.  Time per call in a full
queue of calls (events around each call, median of a window; three windows per arm after a warm-up, the arms alternating on the same GPU in
the same process), as tools/bench_tsdf.py measures: a CALL RATE.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace -d DIR -o mesh -- python tools/bench_tsdf_mesh.py --kernels-only
which launches the `given +normals` form 20 times per grid; --trace DIR/mesh_results.db (the profiler's SQLite output) then adds the median
duration of each of the call's seven kernels and, for the two flag kernels, the algorithmic bytes per second (distance and weight read
once each by the cell flag; the same plus the cell mask by the slot flag).
Prints one JSON line and writes the table to --out (default profiles/tsdf_mesh_bench.txt).
    python tools/bench_tsdf_mesh.py [--out PATH] [--kernels-only] [--trace PATH] [--resources TEXT] [--grids 128,256]"""
import argparse
import json
import os
import sqlite3
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_tsdf  # noqa: E402
from bench_tsdf import alternate, median, same_bits  # noqa: E402
from unidepth_amd import tsdf, tsdfmesh  # noqa: E402

TRACE_CALLS = 20
KERNELS = ("tm_cell_flag_kernel", "cp_scan_tiles_kernel", "cp_scan_batch_kernel", "tm_slot_flag_kernel", "tm_scan_faces_kernel",
           "tm_vert_pack_kernel", "tm_face_pack_kernel")
KEYS = ("vertices", "faces", "rgb", "normals", "vert_counts", "vert_offsets", "face_counts", "face_offsets")
H, W, V = 480, 640, 8


def volume(N):
    """bench_tsdf.py's `mixed+cw` volume of N^3 voxels"""
    fused, _ = bench_tsdf.workloads(N, V, H, W)["mixed+cw"]
    vol, _ = fused()
    torch.cuda.synchronize()
    return vol


def trace_medians(path, n_groups):
    """the kernel trace of a --kernels-only run -> per grid {kernel: median duration (us) of its dispatches}; cp_scan_batch_kernel runs
    twice per call (vertices, faces) and is reported as the sum of both.  Each grid's group also holds the counted call that sizes the
    outputs: a counting pass and a packing pass (the pack kernels run in the second only)."""
    db = sqlite3.connect(path)
    out = [dict() for _ in range(n_groups)]
    for name in KERNELS:
        dur = [r[0] / 1e3 for r in db.execute(f"select duration from kernels where name like '%{name}%' order by start")]
        per_call = 2 if name == "cp_scan_batch_kernel" else 1
        size = (TRACE_CALLS + (1 if "pack" in name else 2)) * per_call
        assert len(dur) == size * n_groups, (name, len(dur), "dispatches in the trace")
        for g in range(n_groups):
            out[g][name] = median(dur[g * size:(g + 1) * size]) * per_call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_mesh_bench.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="launch the given +normals form 20 times per grid and exit (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="mesh_results.db of a --kernels-only run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--resources", default="", help="a line on the compiler's register and scratch report, copied into the table")
    ap.add_argument("--grids", default="128,256", help="the grid sides to run, comma separated")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_mesh.py needs a GPU"
    grids = [int(x) for x in args.grids.split(",")]
    kernel_us = None
    if args.trace:
        try:
            kernel_us = trace_medians(args.trace, len(grids))
        except (OSError, sqlite3.Error, AssertionError) as e:               # the call times do not depend on the trace
            print(f"bench_tsdf_mesh: kernel trace not used ({e!r})", file=sys.stderr)
    res = {"op": "tsdf_mesh (a TSDF volume's surface as an indexed triangle mesh: two ordered compactions)", "windows": bench_tsdf.WINDOWS,
           "window_s": bench_tsdf.WINDOW_S}
    lines = ["tools/bench_tsdf_mesh.py on " + torch.cuda.get_device_name(0) + ": ms per call (a call rate), median of a window of queued calls (n = calls "
             f"per window, as many as fit {bench_tsdf.WINDOW_S} s, 5 .. 200); {bench_tsdf.WINDOWS} windows per arm after a warm-up, tsdf_mesh alternating with",
             "tsdf_mesh_composition (vectorised torch) and with tsdf_points on the same volume; B = 1, bench_tsdf.py's mixed+cw volume (8 views of "
             "480x640); [..] = every window; ratio = tsdf_mesh / yardstick.",
             "kernels = median duration of 20 dispatches in a rocprofv3 --kernel-trace run of its own (given +normals form); GB/s = the algorithmic "
             "bytes of a flag kernel (distance + weight read once, + the cell mask for the slots) over that time." if kernel_us
             else "kernel times: not measured in this run (no --trace).", ""]
    if args.resources:
        lines[-1:] = [args.resources, ""]
    slower = []
    for gi, N in enumerate(grids):
        vol = volume(N)
        counted = tsdfmesh.tsdf_mesh(vol, return_normals=True)
        nv, nf = counted.vertices.shape[0], counted.faces.shape[0]
        given = lambda normals: tsdfmesh.tsdf_mesh(vol, vert_capacity=nv, face_capacity=nf, return_normals=normals)  # noqa: E731
        if args.kernels_only:
            for _ in range(TRACE_CALLS):
                given(True)
            torch.cuda.synchronize()
            continue
        comp = tsdfmesh.tsdf_mesh_composition(vol, return_normals=True)
        equal = all(same_bits(getattr(counted, k), getattr(comp, k)) for k in KEYS)
        g = given(True)
        equal_given = all(same_bits(getattr(counted, k), getattr(g, k)) for k in KEYS)
        points = tsdf.tsdf_points(vol)
        del comp, g
        r = {"vertices": nv, "triangles": nf, "points": int(points.xyz.shape[0]), "bit_equal_composition": equal, "bit_equal_given": equal_given}
        lines.append(f"n{N}  ({N}^3 voxels; {nv} vertices, {nf} triangles; tsdf_points: {points.xyz.shape[0]} points)  bit-equal to the composition {equal}, "
                     f"given == counted {equal_given}")
        arms = {"counted": lambda: tsdfmesh.tsdf_mesh(vol), "counted +normals": lambda: tsdfmesh.tsdf_mesh(vol, return_normals=True),
                "given": lambda: given(False), "given +normals": lambda: given(True)}
        yard = {"composition": lambda: tsdfmesh.tsdf_mesh_composition(vol), "composition +normals": lambda: tsdfmesh.tsdf_mesh_composition(vol, return_normals=True),
                "tsdf_points": lambda: tsdf.tsdf_points(vol), "tsdf_points given": lambda: tsdf.tsdf_points(vol, capacity=int(points.xyz.shape[0]))}
        for arm, other in (("counted", "composition"), ("counted +normals", "composition +normals"), ("given +normals", "composition +normals"),
                           ("counted", "tsdf_points"), ("given", "tsdf_points given")):
            ta, tb, ra, rb = alternate(arms[arm], yard[other])
            ma, mb = median(ta), median(tb)
            r[f"{arm} vs {other}"] = {"mesh_ms": round(ma, 4), "mesh_runs_ms": [round(t, 4) for t in ta], "mesh_calls_per_window": ra,
                                      "yardstick_ms": round(mb, 4), "yardstick_runs_ms": [round(t, 4) for t in tb], "yardstick_calls_per_window": rb,
                                      "ratio": round(ma / mb, 4)}
            if other.startswith("composition") and ma > mb:
                slower.append(f"n{N} {arm}")
            lines.append(f"  {arm:17s} {ma:.4f} {[round(t, 4) for t in ta]} n={ra}  {other:21s} {mb:.4f} {[round(t, 4) for t in tb]} n={rb}  ratio {ma / mb:.4f}")
        if kernel_us:
            k = kernel_us[gi]
            r["kernel_us"] = {name: round(v, 1) for name, v in k.items()}
            vox = N ** 3
            cell_gbs = 8 * vox / (k["tm_cell_flag_kernel"] * 1e-6) / 1e9
            slot_gbs = (8 * vox + vox / 8) / (k["tm_slot_flag_kernel"] * 1e-6) / 1e9
            r["cell_flag_GBps"], r["slot_flag_GBps"] = round(cell_gbs, 1), round(slot_gbs, 1)
            lines.append("  kernels (us): " + ", ".join(f"{name} {v:.1f}" for name, v in k.items()) + f"; sum {sum(k.values()):.1f}")
            lines.append(f"  cell flag {cell_gbs:.0f} GB/s, slot flag {slot_gbs:.0f} GB/s of algorithmic bytes")
        res[f"n{N}"] = r
        lines.append("")
        del vol, counted, points
    if args.kernels_only:
        return
    lines.append("slower than the composition: " + (", ".join(slower) if slower else "no workload"))
    res["slower_than_composition"] = slower
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
