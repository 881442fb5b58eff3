"""Helper of the eval_3d_batch tests (not a conftest: the test modules and tools/make_golden_eval3d.py import it).

A numpy restatement of one whole ud_eval_3d call (include/unidepth_hip.h UdEval3d), operation by operation:

  * the sample size: eval_ops.eval_3d_size (the reference's fp32 rule) and F.interpolate(mode="nearest-exact")'s source indices;
  * the row-major compaction of every image's valid samples (the order of gt[:, mask]);
  * the nearest-neighbour distances: oracle.restate_eval.knn_points (import-only; bit-exact against the reference's own CPU
    implementation by tests/test_oracle_eval_pins.py), each direction once -- a brute-force [n, n] matrix in numpy, a minute per large
    case, so the searches of one call run on a few threads, and a GPU test may pass `knn=` to take the distances of its three large
    cases from ud_knn_points instead (pinned bit-exact to the same restatement by tests/test_eval_ops_gpu.py);
  * integer threshold counts (strict <, fp32, against the squared distance) and fp64 sums;
  * F1 from the integer counts in the kernel's arithmetic (f1_from_counts);

and the seeded inputs of the golden cases (case_inputs, CPU generator), so that any box regenerates them; tests/golden/
eval_3d_batch.npz stores only the REFERENCE's outputs (tools/make_golden_eval3d.py)."""
from __future__ import annotations

import functools
import os
from concurrent.futures import ThreadPoolExecutor
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import restate_eval  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_3d_batch.npz")
KEYS = ("MSE_3d", "chamfer", "F1")
CASES = ("small_t100", "empty_middle", "edge_b8_100", "full_518_b3", "quarter_518_b3", "ties_lattice")
RTOL = 5e-6            # tests/test_eval_ops_gpu.py's tolerance for eval_3d against the same reference


def eval_3d_size(H, W, n_valid):
    from unidepth_amd import eval_ops
    return eval_ops.eval_3d_size(H, W, n_valid)


def _thresholds(min_depth=0.01, max_depth=10.0):
    return torch.linspace(np.log(min_depth), np.log(max_depth / 20), 100).exp()


def _points(g, B, H, W):
    """A smooth surface seen through a pinhole (gt) and a noisy copy of it (pred), as oracle.make_golden_eval.eval3d_case_inputs."""
    z = 1.0 + 4.0 * torch.rand(B, 1, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(-0.6, 0.6, H), torch.linspace(-0.8, 0.8, W), indexing="ij")
    gts = torch.cat([xx[None, None] * z, yy[None, None] * z, z], 1)
    preds = gts * (1.0 + 0.03 * torch.randn(B, 3, H, W, generator=g)) + 0.01 * torch.randn(B, 3, H, W, generator=g)
    return gts, preds


def case_inputs(name: str):
    """(gts [B,3,H,W] f32, preds, masks [B,1,H,W] bool, thresholds: a tensor or a list of floats) of a golden case, CPU tensors."""
    seed = 4100 + CASES.index(name)
    g = torch.Generator().manual_seed(seed)
    if name == "small_t100":                      # no resample; T = 100, thresholds as a tensor
        gts, preds = _points(g, 2, 48, 64)
        return gts, preds, torch.rand(2, 1, 48, 64, generator=g) < 0.8, _thresholds()
    if name == "empty_middle":                    # odd sizes; image 1 has no valid pixel, image 2 exactly one
        gts, preds = _points(g, 3, 37, 53)
        masks = torch.rand(3, 1, 37, 53, generator=g) < 0.7
        masks[1] = False
        masks[2] = False
        masks[2, 0, 17, 29] = True
        return gts, preds, masks, _thresholds().tolist()
    if name == "edge_b8_100":                     # S = 80000: the ratio is just below 1 (97 x 97), almost every source row is sampled
        gts, preds = _points(g, 8, 100, 100)
        return gts, preds, torch.ones(8, 1, 100, 100, dtype=torch.bool), _thresholds().tolist()
    if name == "full_518_b3":                     # S = 804972: 160 x 160 by the fp32 rule (159 with an fp64 product)
        gts, preds = _points(g, 3, 518, 518)
        return gts, preds, torch.ones(3, 1, 518, 518, dtype=torch.bool), _thresholds().tolist()
    if name == "quarter_518_b3":                  # S = 201243 exactly, unevenly spread: 320 x 320 (319 with an fp64 product)
        gts, preds = _points(g, 3, 518, 518)
        masks = torch.zeros(3, 518 * 518, dtype=torch.bool)
        for b, n in enumerate((120000, 60000, 21243)):
            masks[b, torch.randperm(518 * 518, generator=g)[:n]] = True
        assert int(masks.sum()) == 201243
        return gts, preds, masks.view(3, 1, 518, 518), _thresholds().tolist()
    if name == "ties_lattice":                    # integer lattice: squared distances exactly equal to a threshold, so strict <
        gts = torch.randint(0, 16, (2, 3, 40, 40), generator=g).float()
        preds = torch.randint(0, 16, (2, 3, 40, 40), generator=g).float()
        return gts, preds, torch.rand(2, 1, 40, 40, generator=g) < 0.9, [1.0, 2.0, 4.0]
    raise KeyError(name)


MANY_TILES_HW = (518, 518)     # 268,324 samples = 263 tiles of 1024 per image: the scan of an image's tile counts needs its carry


def many_tiles_inputs():
    """A case without a reference golden (so not in CASES): B = 2 at 518 x 518 with about 3,000 valid pixels per image, so the sample
    grid stays the image (S <= 76,800) and has 263 tiles.  Both images have valid pixels in the tiles 0, 255 (the last of the scan's
    first chunk of 256), 256 (the second chunk) and 262 (the last, partial tile); tile 1 of image 1 is empty."""
    H, W = MANY_TILES_HW
    g = torch.Generator().manual_seed(4263)
    gts, preds = _points(g, 2, H, W)
    masks = torch.zeros(2, H * W, dtype=torch.bool)
    for b in range(2):
        masks[b, torch.randperm(H * W, generator=g)[:3000]] = True
        for t in (0, 255, 256, 262):
            masks[b, t * 1024 + 7 * (b + 1)] = True                    # 262 * 1024 + 14 < 518 * 518
    masks[0, 1024 + 500] = True
    masks[1, 1024:2048] = False
    tiles = np.add.reduceat(masks.numpy().astype(np.int64), np.arange(0, H * W, 1024), axis=1)
    assert tiles.shape == (2, 263) and (tiles[:, (0, 255, 256, 262)] > 0).all() and tiles[0, 1] > 0 and tiles[1, 1] == 0
    assert int(masks.sum()) <= 76800 and eval_3d_size(H, W, int(masks.sum())) == (H, W)
    return gts, preds, masks.view(2, 1, H, W), _thresholds().tolist()


def nearest_exact_index(n_in: int, n_out: int) -> np.ndarray:
    """Source index of every output index of F.interpolate(mode="nearest-exact", size=n_out): min(floor((dst + 0.5) * scale), n_in - 1)
    with scale = n_in / n_out and the product in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
    return np.minimum(np.floor(dst * scale).astype(np.int64), n_in - 1)


def f1_from_counts(c1, c2, n: int) -> np.float32:
    """F1 of one image from its integer threshold counts, in ud_eval_3d's arithmetic: p, r, f in fp32 (NaN -> 0), the trapezoid sum
    in fp64 in index order, / T, rounded to fp32 once."""
    T = len(c1)
    p = np.asarray(c1, np.float32) / np.float32(n)
    r = np.asarray(c2, np.float32) / np.float32(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.float32(2.0) * p * r / (p + r)
    f = np.where(np.isnan(f), np.float32(0), f).astype(np.float32)
    area = 0.0
    for t in range(T - 1):
        area += (float(f[t]) + float(f[t + 1])) * 0.5
    return np.float32(area / T)


def _knn_numpy(p1: np.ndarray, p2: np.ndarray) -> np.ndarray:
    """Squared distance of every p1 [n,3] row to its nearest p2 [m,3] row."""
    return restate_eval.knn_points(p1[None], p2[None], K=1)[0][0, :, 0]


def restate(gts, preds, masks, thresholds, knn=None, workers: int = 4) -> dict:
    """The whole call on the CPU: {"size": (h, w), "count": int64 [B], "MSE_3d" / "chamfer" / "F1": f32 [B] (NaN where count is 0),
    "c1" / "c2": int64 [B, T] threshold counts}.  knn(p1 [n,3], p2 [m,3]) -> f32 [n] replaces the numpy search (called serially)."""
    gts = np.ascontiguousarray(torch.as_tensor(gts).float().numpy())
    preds = np.ascontiguousarray(torch.as_tensor(preds).float().numpy())
    B, _, H, W = gts.shape
    masks = torch.as_tensor(masks).reshape(B, H, W).numpy() != 0
    th = torch.as_tensor(thresholds).to(torch.float32).numpy()
    T = th.shape[0]
    S = int(masks.sum())
    h, w = eval_3d_size(H, W, S)
    out = {"size": (h, w), "count": np.zeros(B, np.int64), "c1": np.zeros((B, T), np.int64), "c2": np.zeros((B, T), np.int64)}
    for k in KEYS:
        out[k] = np.full(B, np.nan, np.float32)
    if S == 0 or h == 0 or w == 0:
        return out
    iy, ix = nearest_exact_index(H, h), nearest_exact_index(W, w)
    clouds = {}
    for b in range(B):
        m = masks[b][iy][:, ix]                                        # [h, w]
        out["count"][b] = int(m.sum())
        if out["count"][b]:
            g = np.ascontiguousarray(gts[b][:, iy][:, :, ix][:, m].T)  # [n, 3], row-major order of the valid samples
            p = np.ascontiguousarray(preds[b][:, iy][:, :, ix][:, m].T)
            clouds[b] = (g, p)
    jobs = [(b, d) for b in clouds for d in (0, 1)]                    # each direction once: d1 = gt -> pred, d2 = pred -> gt
    if knn is None:
        with ThreadPoolExecutor(max(1, min(workers, len(jobs)))) as ex:
            dist = dict(zip(jobs, ex.map(lambda j: _knn_numpy(*(clouds[j[0]] if j[1] == 0 else clouds[j[0]][::-1])), jobs)))
    else:
        dist = {j: np.asarray(knn(*(clouds[j[0]] if j[1] == 0 else clouds[j[0]][::-1])), np.float32) for j in jobs}
    for b, (g, p) in clouds.items():
        n = int(out["count"][b])
        d = g - p
        norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d1, d2 = dist[(b, 0)], dist[(b, 1)]
        out["MSE_3d"][b] = np.float32(norm.astype(np.float64).sum() / n)
        out["chamfer"][b] = np.float32(((np.sqrt(d1) + np.sqrt(d2)) / np.float32(2)).astype(np.float64).sum() / n)
        out["c1"][b] = [(d1 < t).sum() for t in th]
        out["c2"][b] = [(d2 < t).sum() for t in th]
        out["F1"][b] = f1_from_counts(out["c1"][b], out["c2"][b], n)
    return out


@functools.lru_cache(maxsize=None)
def restated_case(name: str) -> dict:
    """restate(*case_inputs(name)), computed once per process and shared (treat as read-only)."""
    return restate(*case_inputs(name))


def golden(name: str) -> dict:
    """The reference's eval_3d outputs of a case: {"MSE_3d", "chamfer", "F1"}, each f32 [number of non-empty images]."""
    g = np.load(GOLDEN)
    return {k: g[f"{name}.{k}"] for k in KEYS}
