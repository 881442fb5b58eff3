"""Golden vectors of the splatting side (unidepth_amd/reproject.py): the reference's own project_points and downsample
(unidepth/utils/geometric.py, torch on the CPU) on seeded inputs -> tests/golden/render_depth.npz.

    python tools/make_golden_render_depth.py        (needs the reference tree; only its outputs are written)

This module also holds what the tests share: PP_CASES / pp_inputs(name) and DS_CASES / ds_inputs(name) (seeded CPU torch.Generator
inputs, rebuilt on any machine), restate() -- an independent numpy restatement of ud_splat (include/unidepth_hip.h UdSplat): the per-point
arithmetic in fp32 with every operation rounded separately, the winners of nearest mode by a sort, the means of mean mode in float64 --
and restate_minpool().  Nothing from the reference is imported at module import time.

The project_points inputs are built backwards from the pixel they must land in: a cell index plus a fraction in [0.25, 0.75], so that
the rounding of the reference's matmul (whose summation order is the BLAS library's business) cannot move a point across a cell edge."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_depth.npz")
REF_GEO = os.path.join("unidepth", "utils", "geometric.py")

# name -> (B, N, H, W, skew): N points per image aimed at the cells [-2, W + 2) x [-2, H + 2)
PP_CASES = {
    "pp_b2_n300_12x16": (2, 300, 12, 16, 0.0),
    "pp_b3_n1000_7x9_skew": (3, 1000, 7, 9, 0.3),
    "pp_b1_n64_1x1": (1, 64, 1, 1, 0.0),
}
# name -> (N, H, W, factor)
DS_CASES = {
    "ds_n2_12x16_f2": (2, 12, 16, 2),
    "ds_n1_9x12_f3": (1, 9, 12, 3),
    "ds_n1_8x8_f1": (1, 8, 8, 1),
    "ds_n1_64x128_f64": (1, 64, 128, 64),
}


def pp_inputs(name):
    """(points fp32 [B,N,3], K fp32 [B,3,3], (H, W), cell int64 [B,N,2] = the (column, row) every point was aimed at) of a golden case.
    A tenth of the points have z < 0 (the reference keeps them); cells outside the image are dropped, cells -1 land in 0 (truncation)."""
    B, N, H, W, skew = PP_CASES[name]
    g = torch.Generator().manual_seed(3000 + sorted(PP_CASES).index(name))
    # uniform draws, products and quotients in float64, one rounding to fp32 at the end: the same bits on every machine
    cu = torch.randint(-2, W + 2, (B, N), generator=g).double()
    cv = torch.randint(-2, H + 2, (B, N), generator=g).double()
    fu = 0.25 + 0.5 * torch.rand(B, N, generator=g).double()
    fv = 0.25 + 0.5 * torch.rand(B, N, generator=g).double()
    z = 1.0 + 6.0 * torch.rand(B, N, generator=g).double()
    z = torch.where(torch.rand(B, N, generator=g) < 0.1, -z, z)
    fx = (0.9 * max(W, 4) + 3.0 * torch.rand(B, generator=g).double()).view(B, 1)
    fy = (0.9 * max(W, 4) + 3.0 * torch.rand(B, generator=g).double()).view(B, 1)
    cx = (W / 2.0 + torch.rand(B, generator=g).double() - 0.5).view(B, 1)
    cy = (H / 2.0 + torch.rand(B, generator=g).double() - 0.5).view(B, 1)
    y = (cv + fv - cy) * z / fy
    x = ((cu + fu - cx) * z - skew * y) / fx
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    K[:, 0, 0], K[:, 0, 1], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2], K[:, 2, 2] = fx[:, 0], skew, cx[:, 0], fy[:, 0], cy[:, 0], 1.0
    pts = torch.stack([x, y, z], dim=-1).float()
    return pts.numpy(), K.float().numpy(), (H, W), torch.stack([cu, cv], dim=-1).long().numpy()


def ds_inputs(name):
    """data fp32 [N,1,H,W]: 70 % zeros (holes), the rest in [0.5, 1500): some blocks all holes, some minima beyond 1000."""
    N, H, W, f = DS_CASES[name]
    g = torch.Generator().manual_seed(4000 + sorted(DS_CASES).index(name))
    r = torch.rand(N, 1, H, W, generator=g)
    v = 0.5 + 1499.5 * (r * r * r)                  # products only: pow rounds differently from one CPU's vector library to the next
    v = torch.where(torch.rand(N, 1, H, W, generator=g) < 0.7, torch.zeros(()), v).float()
    return v.numpy(), f


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _np(x):
    return None if x is None else np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def split_packed(rows, offsets, n_rows=None):
    """Packed rows [n,C] + offsets [B+1] -> the per-image arrays ud_splat sees: image b owns rows [offsets[b], min(offsets[b+1], n))."""
    rows, offsets = _np(rows), _np(offsets)
    n = rows.shape[0] if n_rows is None else n_rows
    return [rows[min(int(offsets[b]), n):min(int(offsets[b + 1]), n)] for b in range(len(offsets) - 1)]


def cells(clouds, K, image_shape, T=None, pixel_offset=0.0, rounding="floor"):
    """The per-point arithmetic of ud_splat: for every image (pixel int64 [n] = row * W + column or -1, z' fp32 [n])."""
    f32 = np.float32
    H, W = image_shape
    K = _np(K).astype(f32).reshape(-1, 3, 3)
    T = None if T is None else _np(T).astype(f32).reshape(-1, 3, 4)
    off = f32(pixel_offset)
    out = []
    with np.errstate(all="ignore"):
        for b, p in enumerate(clouds):
            p = _np(p).astype(f32)
            x, y, z = (np.ascontiguousarray(p[:, c]) for c in range(3))
            if T is not None:
                t = T[b if T.shape[0] > 1 else 0]
                x, y, z = [((t[r, 0] * x + t[r, 1] * y) + t[r, 2] * z) + t[r, 3] for r in range(3)]
            k = K[b if K.shape[0] > 1 else 0]
            a, b_, w = [(k[r, 0] * x + k[r, 1] * y) + k[r, 2] * z for r in range(3)]
            u, v = a / w + off, b_ / w + off
            assert u.dtype == f32 and v.dtype == f32 and z.dtype == f32
            ok = np.ones(x.shape, dtype=bool)
            idx = []
            for c, n in ((u, W), (v, H)):
                f = np.trunc(c) if rounding == "trunc" else np.floor(c)
                good = (f >= 0) & (f < f32(2147483648.0))          # decided in float: NaN and infinities fail, -0.0 passes
                i = np.where(good, f, 0).astype(np.int64)
                ok &= good & (i < n)
                idx.append(i)
            out.append((np.where(ok, idx[1] * W + idx[0], -1), z))
    return out


def restate(clouds, K, image_shape, T=None, mode="nearest", pixel_offset=0.0, rounding="floor", depth_range=None, colors=None):
    """ud_splat restated on a list of per-image clouds [n_b,3] (colors: a list of [n_b,3] arrays or None) -> dict of depth [B,H,W] (fp32
    bits of the winner in nearest mode, the float64 mean in mean mode, NaN at 2^19 points or more), index int32 [B,H,W] (-1 = hole;
    nearest), rgb [B,3,H,W] or None (nearest), count int32 [B,H,W], abs_sum float64 [B,H,W] (sum of |z'| per pixel; mean mode's bound)."""
    f32 = np.float32
    H, W = image_shape
    B = len(clouds)
    depth = np.zeros((B, H * W), dtype=f32 if mode == "nearest" else np.float64)
    index = np.full((B, H * W), -1, dtype=np.int32)
    count = np.zeros((B, H * W), dtype=np.int32)
    abs_sum = np.zeros((B, H * W), dtype=np.float64)
    rgb = None if colors is None else np.zeros((B, 3, H * W), dtype=_np(colors[0]).dtype)
    for b, (pix, z) in enumerate(cells(clouds, K, image_shape, T, pixel_offset, rounding)):
        keep = pix >= 0
        with np.errstate(all="ignore"):
            if depth_range is not None:
                keep &= (z >= f32(depth_range[0])) & (z <= f32(depth_range[1]))
            keep &= (z > 0) if mode == "nearest" else (np.abs(z) <= f32(2.0 ** 20))
        r = np.nonzero(keep)[0]
        pk, zk = pix[r], z[r]
        count[b] = np.bincount(pk, minlength=H * W)
        if mode == "nearest":
            order = np.lexsort((r, zk.view(np.uint32), pk))      # by pixel, then z' (positive: its bits order like its value), then index
            first = order[np.concatenate([[True], pk[order][1:] != pk[order][:-1]])] if r.size else order
            depth[b, pk[first]] = zk[first]
            index[b, pk[first]] = r[first]
            if rgb is not None:
                rgb[b][:, pk[first]] = _np(colors[b])[r[first]].T
        else:
            s = np.bincount(pk, weights=zk.astype(np.float64), minlength=H * W)
            abs_sum[b] = np.bincount(pk, weights=np.abs(zk).astype(np.float64), minlength=H * W)
            depth[b] = np.where(count[b] > 0, s / np.maximum(count[b], 1), 0.0)
            depth[b, count[b] >= 2 ** 19] = np.nan
    shape = (B, H, W)
    return {"depth": depth.reshape(shape), "index": index.reshape(shape), "count": count.reshape(shape), "abs_sum": abs_sum.reshape(shape),
            "rgb": None if rgb is None else rgb.reshape(B, 3, H, W)}


def restate_minpool(data, f):
    """ud_depth_minpool restated: [N,1,H,W] fp32 -> [N,1,H/f,W/f]; zeros count as 1e5, a minimum beyond 1000 is written as 0."""
    data = _np(data).astype(np.float32)
    N, _, H, W = data.shape
    blocks = data.reshape(N, H // f, f, W // f, f).transpose(0, 1, 3, 2, 4).reshape(N, H // f, W // f, f * f)
    m = np.where(blocks == 0, np.float32(1e5), blocks).min(axis=-1)          # ndarray.min propagates a NaN, as torch.min
    return np.where(m > np.float32(1000.0), np.float32(0.0), m).astype(np.float32).reshape(N, 1, H // f, W // f)


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_path():
    """geometric.py in the reference tree (oracle/ref_loader.py REF_ROOT; present on the authoring machine only)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return os.path.join(ref_loader.REF_ROOT, REF_GEO)


def reference_module():
    """The reference's geometric module (it imports torch only), loaded from the reference tree."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ref_geometric", reference_path())
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_outputs(ref):
    """name -> array for every case: the reference's mean-depth maps, the cell its project_points puts EACH point in (one call per image
    on a batch of N one-point clouds: the only non-zero pixel of map i is point i's; -1 when it lands nowhere), and its downsample."""
    out = {}
    for name in PP_CASES:
        pts, K, (H, W), _ = pp_inputs(name)
        out[name] = ref.project_points(torch.from_numpy(pts), torch.from_numpy(K), (H, W)).numpy()
        cell = np.full(pts.shape[:2], -1, dtype=np.int32)
        for b in range(pts.shape[0]):
            one = ref.project_points(torch.from_numpy(pts[b][:, None, :].copy()), torch.from_numpy(K[b:b + 1]).repeat(pts.shape[1], 1, 1), (H, W))
            flat = one.reshape(pts.shape[1], H * W) != 0
            assert (flat.sum(dim=1) <= 1).all()
            cell[b] = torch.where(flat.any(dim=1), flat.int().argmax(dim=1), torch.tensor(-1)).numpy()
        out[name + "_cell"] = cell
    for name in DS_CASES:
        data, f = ds_inputs(name)
        out[name] = ref.downsample(torch.from_numpy(data), f).numpy()
    return out


def main():
    out = reference_outputs(reference_module())
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
