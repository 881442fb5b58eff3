"""Golden vectors of match_gt / match_intrinsics (unidepth_amd/matching.py, csrc/matchgt.hip): the reference's own functions
(unidepth/utils/misc.py, torch on the CPU) on seeded inputs -> tests/golden/match_gt.npz.

    python tools/make_golden_match_gt.py          (needs the reference tree; only its outputs are written)

This module also holds what the tests share: CASES / case_inputs(name) (seeded CPU torch.Generator inputs, uniform draws only, the same
bits on every machine) and an independent numpy restatement of ud_match_gt (include/unidepth_hip.h UdMatchGt):
restate(..., dtype=np.float32) rounds every operation separately in fp32 -- the kernel's definition, reproduced bit for bit --
and restate(..., dtype=np.float64) is the same expression in fp64 on fp64 coordinates, the value the error bounds are measured from.
Nothing from the reference is imported at module import time."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "match_gt.npz")
REF_MISC = os.path.join("unidepth", "utils", "misc.py")

# name -> (B, C, h1, w1, H2, W2, target paddings too, stored in the golden file).  The large shapes are rebuilt and restated by the
# tests but not stored (one 375 x 1242 plane alone is 1.8 MB).
CASES = {
    "up_28x42_37x53": (2, 2, 28, 42, 37, 53, False, True),
    "down_42x56_20x31": (3, 1, 42, 56, 20, 31, False, True),
    "mixed_14x70_33x17_pads2": (2, 1, 14, 70, 33, 17, True, True),
    "up_28x42_63x257_pads2": (1, 1, 28, 42, 63, 257, True, True),
    "up_98x126_480x640": (2, 1, 98, 126, 480, 640, False, False),
    "kitti_518x518_375x1242": (1, 1, 518, 518, 375, 1242, True, False),
}
GOLDEN_CASES = [n for n, c in CASES.items() if c[7]]


def case_inputs(name):
    """(src fp32 [B,C,h1,w1], pads1 int64 [B,4] lrtb, pads2 int64 [B,4] or None, K fp32 [B,3,3], (H2, W2)) of a case, numpy."""
    B, C, h1, w1, H2, W2, with_p2, _ = CASES[name]
    g = torch.Generator().manual_seed(4100 + sorted(CASES).index(name))
    src = (5.0 * torch.rand(B, C, h1, w1, generator=g) - 1.0).float()           # both signs: sums of taps can cancel
    pads1 = torch.stack([torch.randint(0, w1 // 3 + 1, (B,), generator=g), torch.randint(0, w1 // 3 + 1, (B,), generator=g),
                         torch.randint(0, h1 // 3 + 1, (B,), generator=g), torch.randint(0, h1 // 3 + 1, (B,), generator=g)], dim=1)
    pads2 = None
    if with_p2:
        pads2 = torch.stack([torch.randint(0, W2 // 4 + 1, (B,), generator=g), torch.randint(0, W2 // 4 + 1, (B,), generator=g),
                             torch.randint(0, H2 // 4 + 1, (B,), generator=g), torch.randint(0, H2 // 4 + 1, (B,), generator=g)], dim=1)
    f = 0.8 * w1 + 4.0 * torch.rand(B, 2, generator=g)
    c = torch.tensor([w1 / 2.0, h1 / 2.0]) + 3.0 * torch.rand(B, 2, generator=g) - 1.5
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f[:, 0], f[:, 1], c[:, 0], c[:, 1], 1.0
    K[:, 0, 1] = 0.25                                                            # a skew entry: copied, never scaled
    return src.numpy(), pads1.numpy(), None if pads2 is None else pads2.numpy(), K.numpy(), (H2, W2)


# ---- restatement of the definitions (numpy) --------------------------------------------------------------------------------------

def _pads(p, B):
    if p is None:
        return np.zeros((B, 4), dtype=np.int64)
    p = np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p, dtype=np.int64).reshape(-1, 4)
    assert p.shape[0] == B, (p.shape, B)
    return p


def axis_weights(n, n2, dtype):
    """Source index pair and weights of the n2 destination samples over n source samples (align_corners=False, source coordinate
    clamped at 0): (i0, i1, low weight, high weight), every operation in `dtype`."""
    dt = np.dtype(dtype).type
    o = np.arange(n2).astype(dtype)
    s = dt(n) / dt(n2)
    f = s * (o + dt(0.5)) - dt(0.5)
    f = np.where(f < dt(0), dt(0), f).astype(dtype)
    i0 = np.minimum(f.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    lo = np.minimum(np.maximum(f - i0.astype(dtype), dt(0)), dt(1)).astype(dtype)
    hi = (dt(1) - lo).astype(dtype)
    return i0, i1, lo, hi


def restate(src, H2, W2, pads1=None, pads2=None, mul=None, B=None, dtype=np.float32, what="value"):
    """ud_match_gt on one plane: src [B or 1, C, h1, w1] (one source broadcasts over `B` images), mul [B,1,h1,w1] or None ->
    [B, C, H2, W2] in `dtype`.  what = "value": the resampled map; "tapsum": the sum of the four taps' absolute values per destination
    pixel (the quantity a coordinate error multiplies)."""
    src = np.asarray(src.cpu() if isinstance(src, torch.Tensor) else src)
    mul = None if mul is None else np.asarray(mul.cpu() if isinstance(mul, torch.Tensor) else mul)
    B = B or (mul.shape[0] if mul is not None else src.shape[0])
    nb, C, h1, w1 = src.shape
    assert nb in (1, B)
    p1, p2 = _pads(pads1, B), _pads(pads2, B)
    out = np.zeros((B, C, H2, W2), dtype=dtype)
    for b in range(B):
        pl, pr, pt, pb = (int(v) for v in p1[b])
        ql, qr, qt, qb = (int(v) for v in p2[b])
        hu, wu, h2, w2 = h1 - pt - pb, w1 - pl - pr, H2 - qt - qb, W2 - ql - qr
        assert hu >= 1 and wu >= 1 and h2 >= 1 and w2 >= 1 and min(pl, pr, pt, pb, ql, qr, qt, qb) >= 0
        v = src[b if nb > 1 else 0].astype(dtype)[:, pt:h1 - pb, pl:w1 - pr]
        if mul is not None:
            v = (v * mul[b].astype(dtype)[:, pt:h1 - pb, pl:w1 - pr]).astype(dtype)
        if hu == h2 and wu == w2 and what == "value":
            res = v
        else:
            y0, y1, ly, hy = axis_weights(hu, h2, dtype)
            x0, x1, lx, hx = axis_weights(wu, w2, dtype)
            v00, v01 = v[:, y0][:, :, x0], v[:, y0][:, :, x1]
            v10, v11 = v[:, y1][:, :, x0], v[:, y1][:, :, x1]
            if what == "tapsum":
                res = np.abs(v00) + np.abs(v01) + np.abs(v10) + np.abs(v11)
            else:
                t0 = (v00 * hx).astype(dtype) + (v01 * lx).astype(dtype)
                t1 = (v10 * hx).astype(dtype) + (v11 * lx).astype(dtype)
                res = (t0 * hy[:, None]).astype(dtype) + (t1 * ly[:, None]).astype(dtype)
        out[b, :, qt:H2 - qb, ql:W2 - qr] = res
    return out


def restate_intrinsics(K, shape1, shape2, pads1=None, pads2=None):
    """The intrinsics part of ud_match_gt: K fp32 [B,3,3], shape1 = (h1, w1), shape2 = (H2, W2) -> fp32 [B,3,3]."""
    f32 = np.float32
    K = np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K).astype(f32).reshape(-1, 3, 3)
    B = K.shape[0]
    p1, p2 = _pads(pads1, B), _pads(pads2, B)
    (h1, w1), (H2, W2) = shape1, shape2
    out = K.copy()
    for b in range(B):
        pl, pr, pt, pb = (int(v) for v in p1[b])
        ql, qr, qt, qb = (int(v) for v in p2[b])
        sx = f32(float(W2 - ql - qr) / float(w1 - pl - pr))
        sy = f32(float(H2 - qt - qb) / float(h1 - pt - pb))
        out[b, 0, 0] = K[b, 0, 0] * sx
        out[b, 1, 1] = K[b, 1, 1] * sy
        out[b, 0, 2] = f32(f32(K[b, 0, 2] - f32(pl)) * sx) + f32(ql)
        out[b, 1, 2] = f32(f32(K[b, 1, 2] - f32(pt)) * sy) + f32(qt)
    return out


def torch_composition(src, H2, W2, pads1=None, pads2=None):
    """What a user of the engine writes without match_gt: per image slice, F.interpolate, F.pad, cat (torch tensors in and out)."""
    import torch.nn.functional as F
    B = src.shape[0]
    h1, w1 = src.shape[-2:]
    p1, p2 = _pads(pads1, B), _pads(pads2, B)
    outs = []
    for b in range(B):
        pl, pr, pt, pb = (int(v) for v in p1[b])
        ql, qr, qt, qb = (int(v) for v in p2[b])
        win = src[b:b + 1, :, pt:h1 - pb, pl:w1 - pr]
        res = F.interpolate(win, size=(H2 - qt - qb, W2 - ql - qr), mode="bilinear")
        outs.append(F.pad(res, (ql, qr, qt, qb)))
    return torch.cat(outs)


# ---- the reference, loaded on demand ---------------------------------------------------------------------------------------------

def reference_path():
    """misc.py in the reference tree (oracle/ref_loader.py REF_ROOT; present on the authoring machine only)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return os.path.join(ref_loader.REF_ROOT, REF_MISC)


def reference_functions():
    """The reference's (match_gt, match_intrinsics), their module loaded from the reference tree by file path."""
    import importlib.util
    sys.dont_write_bytecode = True                       # the reference tree is read-only
    spec = importlib.util.spec_from_file_location("_ref_misc", reference_path())
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.match_gt, mod.match_intrinsics


def reference_output(fns, name):
    """(matched map fp32 [B,C,H2,W2], matched K fp32 [B,3,3]) of a case from the reference's functions, numpy."""
    match_gt, match_intrinsics = fns
    src, pads1, pads2, K, (H2, W2) = case_inputs(name)
    t1 = torch.from_numpy(src)
    t2 = torch.zeros(src.shape[0], 1, H2, W2)
    # paddings as lists of int tuples (the documented argument type): the scale factors of match_intrinsics are then Python floats,
    # the correctly rounded quotients.  With tensor paddings `int / tensor` goes through torch's reciprocal-and-multiply instead.
    p1 = [tuple(int(v) for v in row) for row in pads1]
    p2 = None if pads2 is None else [tuple(int(v) for v in row) for row in pads2]
    out = match_gt(t1, t2, padding1=p1, padding2=p2)
    Kn = match_intrinsics(torch.from_numpy(K), t1, t2, padding1=p1, padding2=p2)
    assert out.dtype == torch.float32 and tuple(out.shape) == (src.shape[0], src.shape[1], H2, W2) and Kn.dtype == torch.float32
    return out.numpy(), Kn.numpy()


def main():
    fns = reference_functions()
    out = {}
    for name in GOLDEN_CASES:
        out[name + ".out"], out[name + ".K"] = reference_output(fns, name)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, f"({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
