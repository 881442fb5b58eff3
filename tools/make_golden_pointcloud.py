"""Golden vectors of the point-cloud packing (unidepth_amd/pointcloud.py): the reference's own get_pointcloud_from_rgbd
(unidepth/utils/visualization.py, numpy on the CPU) on seeded inputs -> tests/golden/pointcloud.npz.

    python tools/make_golden_pointcloud.py          (needs the reference tree; only its outputs are written)

This module also holds what the tests share: CASES / case_inputs(name) (seeded CPU torch.Generator inputs, rebuilt on any machine) and
restate() -- an independent numpy restatement of ud_pointcloud_pack's predicate (compares and the edge test in fp32, every operation
rounded separately) and of both coordinate modes (points copied; depth-mode x, y in float64, the reference's precision), which the GPU
tests use where there is no golden file.  Nothing from the reference is imported at module import time."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointcloud.npz")
REF_VIS = os.path.join("unidepth", "utils", "visualization.py")

# name -> (H, W, fraction of the mask that is set)
CASES = {
    "rgbd_24x31_mask60": (24, 31, 0.6),
    "rgbd_23x32_mask5": (23, 32, 0.05),
    "rgbd_25x30_full": (25, 30, 1.0),
}


def case_inputs(name):
    """(image u8 [H,W,3], depth fp32 [H,W], mask bool [H,W], K fp32 [3,3]) of a golden case, numpy."""
    H, W, frac = CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    # uniform draws and one multiply-add only: exp / log / randn round differently from one CPU's vector library to the next, and the
    # golden z column is this array bit for bit
    depth = (1.0 + 6.0 * torch.rand(H, W, generator=g)).float()
    mask = torch.rand(H, W, generator=g) < frac if frac < 1.0 else torch.ones(H, W, dtype=torch.bool)
    f = 0.9 * W + torch.rand(2, generator=g) * 3.0
    c = torch.tensor([W / 2.0, H / 2.0]) + torch.rand(2, generator=g) - 0.5
    K = torch.tensor([[f[0], 0.0, c[0]], [0.0, f[1], c[1]], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return image.numpy(), depth.numpy(), mask.numpy(), K.numpy()


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _np(x):
    return None if x is None else np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def valid_mask(points=None, depth=None, mask=None, confidence=None, min_confidence=None, depth_range=None, edge_rtol=None):
    """The predicate of ud_pointcloud_pack (include/unidepth_hip.h) on [B,...] arrays -> bool [B,H,W].  fp32 compares."""
    points, depth, mask, confidence = _np(points), _np(depth), _np(mask), _np(confidence)
    f32 = np.float32
    if depth is not None:
        d = depth.reshape(depth.shape[0], depth.shape[-2], depth.shape[-1]).astype(f32)
    else:
        d = points[:, 2].astype(f32)
    B, H, W = d.shape
    with np.errstate(all="ignore"):
        v = np.ones((B, H, W), dtype=bool)
        if mask is not None:
            v &= mask.reshape(B, H, W) != 0
        if points is not None:
            v &= np.isfinite(points).all(axis=1)
        else:
            v &= np.isfinite(d)
        if min_confidence is not None:
            v &= confidence.reshape(B, H, W).astype(f32) >= f32(min_confidence)
        if depth_range is not None:
            v &= (d >= f32(depth_range[0])) & (d <= f32(depth_range[1]))
        if edge_rtol is not None:
            def ok(a, n):                   # a NaN on either side makes the compare false (np.fmin returns the other operand, as fminf)
                return np.abs(a - n) <= f32(edge_rtol) * np.fmin(a, n)
            e = np.ones((B, H, W), dtype=bool)
            e[:, :, 1:] &= ok(d[:, :, 1:], d[:, :, :-1])
            e[:, :, :-1] &= ok(d[:, :, :-1], d[:, :, 1:])
            e[:, 1:, :] &= ok(d[:, 1:, :], d[:, :-1, :])
            e[:, :-1, :] &= ok(d[:, :-1, :], d[:, 1:, :])
            v &= e
    return v


def restate(points=None, depth=None, K=None, image=None, mask=None, confidence=None, min_confidence=None, depth_range=None,
            edge_rtol=None, flip_y=False):
    """ud_pointcloud_pack restated: dict of xyz [N,3] (fp32 copies in points mode, float64 in depth mode), rgb [N,3] (image's dtype) or
    None, index int32 [N], counts int64 [B], offsets int64 [B+1], valid bool [B,H,W].  Rows: images in batch order, pixels row-major."""
    points, depth, K, image = _np(points), _np(depth), _np(K), _np(image)
    v = valid_mask(points, depth, mask, confidence, min_confidence, depth_range, edge_rtol)
    B, H, W = v.shape
    bb, yy, xx = np.nonzero(v)                                # row-major: batch, then rows, then columns
    if points is not None:
        xyz = np.stack([points[bb, c, yy, xx] for c in range(3)], axis=-1).astype(np.float32)
    else:
        d = depth.reshape(B, H, W)[bb, yy, xx].astype(np.float64)
        Kb = K.reshape(-1, 3, 3).astype(np.float64)
        Kb = Kb[bb] if Kb.shape[0] > 1 else np.broadcast_to(Kb[0], (bb.size, 3, 3))
        x = (xx - Kb[:, 0, 2]) * d / Kb[:, 0, 0]
        y = (yy - Kb[:, 1, 2]) * d / Kb[:, 1, 1]
        xyz = np.stack([x, y, d], axis=-1)
    if flip_y:
        xyz[:, 1] = -xyz[:, 1]
    rgb = None if image is None else np.stack([image[bb, c, yy, xx] for c in range(3)], axis=-1)
    counts = v.reshape(B, -1).sum(axis=1).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return {"xyz": xyz, "rgb": rgb, "index": (yy * W + xx).astype(np.int32), "counts": counts, "offsets": offsets, "valid": v}


def restate_rgbd(image, depth, mask, K):
    """get_pointcloud_from_rgbd restated on one image ([H,W,C], [H,W], [H,W], [3,3]) -> float64 [N, 3 + C], +y up."""
    r = restate(depth=depth[None], K=K, mask=mask[None], flip_y=True)
    colours = np.asarray(image).reshape(depth.size, -1)[r["index"].astype(np.int64)]
    return np.concatenate([r["xyz"], colours], axis=-1)


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_path():
    """visualization.py in the reference tree (oracle/ref_loader.py REF_ROOT; present on the authoring machine only)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return os.path.join(ref_loader.REF_ROOT, REF_VIS)


def reference_get_pointcloud_from_rgbd():
    """The reference's get_pointcloud_from_rgbd, its module loaded from the reference tree with stand-ins for the plotting / logging
    imports it makes at import time (none is used by the function)."""
    import importlib.util
    names = ("matplotlib", "matplotlib.pyplot", "wandb", "PIL", "PIL.Image", "unidepth", "unidepth.utils", "unidepth.utils.misc")
    saved = {k: sys.modules.get(k) for k in names}
    for k in names:
        sys.modules[k] = types.ModuleType(k)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    sys.modules["unidepth.utils.misc"].ssi_helper = None
    try:
        spec = importlib.util.spec_from_file_location("_ref_visualization", reference_path())
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.get_pointcloud_from_rgbd


def reference_output(ref_fn, name):
    image, depth, mask, K = case_inputs(name)
    out = np.asarray(ref_fn(image, depth, mask, K))
    # a mask without a False shrinks to numpy's `nomask` inside the reference, whose boolean index then adds an axis: [1,H,W,6], the
    # same rows in the same order; stored as [N,6] like the others
    assert out.dtype == np.float64 and out.shape[-1] == 6 and (out.ndim == 2 or mask.all()), (out.dtype, out.shape)
    return out.reshape(-1, 6)


def main():
    ref = reference_get_pointcloud_from_rgbd()
    out = {name: reference_output(ref, name) for name in CASES}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
