"""Camera tracking against a model view: frame-to-model projective point-to-plane ICP, the step of a KinectFusion-style loop that turns
tsdf_render's surface prediction and a new depth frame into the frame's pose -- infer() -> track_camera against volume.render(...) ->
tsdf_integrate with the pose found, all on the device.

    icp_linearize(frame, camera, model_points, model_normals, model_valid, model_camera, transform, ...)
                                            the 6 x 6 normal system of one Gauss-Newton step, fp64 [B,32]: ud_icp_linearize (csrc/icp.hip)
    icp_solve(system, transform, ...)       LDL^T and the Cayley retraction on the device: ud_icp_update
    track_camera(frame, camera, ..., iters=10)     iters steps on one T buffer, two launches each
    icp_linearize_composition, track_camera_composition    the same definition spelled with gt_points / unproject_camera,
                                            project_camera, remap(mode="nearest") and torch: the oracle of the fused kernels' tests
    TsdfVolume.track(...)                   render at the prior pose, then track_camera (tsdf.py)

For every frame pixel: its point p moved by the estimate, q = T p (frame camera -> model camera), projected through the model camera; the
model's point m and normal n read at the nearest pixel; the residual r = n . (m - q) and the row g = (q x n, n).  The pixel is matched
when it is live, q lands in the model image in front of the camera on a valid model pixel with a non-zero normal, |m - q| <= dist_tol and
(with frame normals and cos_tol) the rotated frame normal agrees with n.  The update x = (omega, v) minimises sum w (r - g . x)^2: A x = b
with A = sum w g g^T, b = sum w g r, summed in fp64 in a fixed order -- bit-reproducible, no atomics.  The HIP kernels are the only
implementation of the fused form: CPU tensors raise."""
from __future__ import annotations

import math
import struct
from typing import Optional

import torch

from . import _args, _lib
from .gtpoints import PreparedCamera, gt_points, prepare_camera
from .ops import check, cur_stream, mk
from .remap import remap
from .reproject import project_camera

SLOTS = 32                 # UD_ICP_SLOTS: A's upper triangle row-major 0..20, b 21..26, e 27, wsum 28, count 29, two zeros
_TRI = [(i, j) for i in range(6) for j in range(i, 6)]
# how ud_icp_linearize runs: the workgroups per image that share the pixels (0: the default, min(ceil(H * W / 256), 256); at most 1024).
# The per-pixel outputs do not depend on it; the sums' last bits do (another order).  tools/bench_icp.py measures 256, 512 and 1024
# (profiles/icp_bench.txt).
_LAUNCH_OPTIONS = dict(blocks=0)


def _f64_bits(v: float) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _damping(fn, damping, min_count):
    try:
        dm = float(damping)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: damping must be a number") from None
    if isinstance(damping, bool) or not (dm >= 0.0 and math.isfinite(dm)):
        raise ValueError(f"{fn}: damping must be finite and not negative, got {damping}")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 0 or min_count >= 2 ** 31:
        raise ValueError(f"{fn}: min_count must be a non-negative integer, got {min_count!r}")
    return dm


def _map3(fn, name, t, B, H, W):
    _args.float_tensor(fn, name, t)
    if tuple(t.shape) != (B, 3, H, W):
        raise ValueError(f"{fn}: {name} {tuple(t.shape)} is not [{B},3,{H},{W}]")


def _arguments(fn, frame, camera, model_points, model_normals, model_valid, model_camera, transform, dist_tol, cos_tol, normals, mask, weights,
               need_T=True):
    """every check the functions share -> the sizes, the tolerances and the tensors in the layout of the descriptor"""
    _args.float_tensor(fn, "frame", frame)
    is_points = frame.ndim == 4 and frame.shape[1] == 3
    B, H, W = _args.point_map(fn, "frame", frame) if is_points else _args.depth_map(fn, "frame", frame)
    _args.max_images(fn, B)
    if not is_points:
        if camera is None:
            raise ValueError(f"{fn}: camera is required with a depth frame (a [B,3,H,W] point map needs none)")
        _args.batch_of(fn, "camera", _args.n_cameras(camera), B, shared=not isinstance(camera, PreparedCamera))
    Bm, Hm, Wm = _args.point_map(fn, "model_points", model_points)
    _args.batch_of(fn, "model_points", Bm, B, shared=False)
    _map3(fn, "model_normals", model_normals, B, Hm, Wm)
    _args.image_map(fn, "model_valid", model_valid, Hm, Wm, mask=True, B=B, shared=False)
    if model_camera is None:
        raise ValueError(f"{fn}: model_camera must be a camera for {B} images")
    _args.batch_of(fn, "model_camera", _args.n_cameras(model_camera), B, shared=not isinstance(model_camera, PreparedCamera))
    _args.max_elems(fn, f"frame={H}x{W} model={Hm}x{Wm}", 6 * H * W, 3 * Hm * Wm)
    if transform is None and need_T:
        raise ValueError(f"{fn}: transform must be fp32 [3,4], [4,4], [1,..] or [{B},..]")
    T, _ = _args.rigid(fn, transform, B)
    tol, tol_bits = _args.tolerance(fn, "dist_tol", dist_tol)
    if isinstance(dist_tol, bool):
        raise ValueError(f"{fn}: dist_tol must be a number, got {dist_tol}")
    has_cos = cos_tol is not None
    cos, cos_bits = 0.0, 0
    if has_cos:
        try:
            cos_bits = _args.f32_bits(float(cos_tol))
        except (TypeError, ValueError, OverflowError, struct.error):
            raise ValueError(f"{fn}: cos_tol must be a number in -1 .. 1") from None
        cos = struct.unpack("<f", struct.pack("<i", cos_bits))[0]
        if isinstance(cos_tol, bool) or not -1.0 <= cos <= 1.0:
            raise ValueError(f"{fn}: cos_tol must be a number in -1 .. 1, got {cos_tol}")
        if normals is None:
            raise ValueError(f"{fn}: cos_tol needs the frame's normals")
    if normals is not None:
        _map3(fn, "normals", normals, B, H, W)
    if mask is not None:
        _args.image_map(fn, "mask", mask, H, W, mask=True, B=B, shared=False)
    if weights is not None:
        _args.image_map(fn, "weights", weights, H, W, mask=False, B=B, shared=False)
    dev = frame.device
    cams = [c for c in (None if is_points else camera, model_camera) if c is not None]
    _args.one_gpu(fn, dev, model_points, model_normals, model_valid, T, normals, mask, weights, *_args.prepared_rows(*cams))
    with torch.cuda.device(dev):
        a = dict(B=B, H=H, W=W, Hm=Hm, Wm=Wm, dev=dev, tol=tol, tol_bits=tol_bits, has_cos=has_cos, cos=cos, cos_bits=cos_bits, T=T)
        a["mcam"] = prepare_camera(model_camera, B, dev)
        a["cam"], a["depth"], a["points"] = None, None, None
        if is_points:
            a["points"] = frame.float().contiguous()
        else:
            a["cam"] = prepare_camera(camera, B, dev)
            a["depth"] = frame.reshape(B, 1, H, W).float().contiguous()
        a["mp"], a["mn"] = model_points.float().contiguous(), model_normals.float().contiguous()
        a["mv"] = model_valid.reshape(B, 1, Hm, Wm).contiguous().view(torch.uint8)
        a["normals"] = None if normals is None else normals.float().contiguous()
        a["mask"] = None if mask is None else mask.reshape(B, 1, H, W).contiguous().view(torch.uint8)
        a["weights"] = None if weights is None else weights.reshape(B, 1, H, W).float().contiguous()
    return a


def _tol2(tol):
    try:
        return struct.unpack("<f", struct.pack("<f", tol * tol))[0]                 # the product of two fp32 values rounded once to fp32
    except OverflowError:
        return math.inf


# ---- the composition ---------------------------------------------------------------------------------------------------------------

def _compose_rows(a, T):
    """-> matched bool [B,1,H,W], residual fp32 [B,1,H,W], rows fp32 [B,6,H,W] (not yet zeroed where unmatched), w fp32 or None"""
    B, dev = a["B"], a["dev"]
    if a["points"] is not None:
        P = a["points"]
        live = torch.isfinite(P).all(dim=1, keepdim=True)
    else:
        P = gt_points(a["depth"], a["cam"])
        live = a["depth"] > 0
    if a["mask"] is not None:
        live = live & a["mask"].bool()
    w = a["weights"]
    if w is not None:
        live = live & (w > 0) & torch.isfinite(w)
    t = [[T[:, r, c].reshape(-1, 1, 1) for c in range(4)] for r in range(3)]
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    q = [((t[r][0] * p0 + t[r][1] * p1) + t[r][2] * p2) + t[r][3] for r in range(3)]         # ud_cam_move's association
    Q = torch.stack(q, dim=1).expand(B, -1, -1, -1).contiguous()
    uv, inside, dq = project_camera(Q, a["mcam"], (a["Hm"], a["Wm"]))
    usable = inside & (dq > 0)
    src = torch.cat([a["mp"], a["mn"]], dim=1)
    mn, valid = remap(src, uv, mode="nearest", coord_valid=usable, src_mask=a["mv"], return_mask=True)
    m, n = mn[:, 0:3], mn[:, 3:6]
    q0, q1, q2 = Q[:, 0], Q[:, 1], Q[:, 2]
    e0, e1, e2 = m[:, 0] - q0, m[:, 1] - q1, m[:, 2] - q2
    d2 = (e0 * e0 + e1 * e1) + e2 * e2
    r = (n[:, 0] * e0 + n[:, 1] * e1) + n[:, 2] * e2
    c0, c1, c2 = q1 * n[:, 2] - q2 * n[:, 1], q2 * n[:, 0] - q0 * n[:, 2], q0 * n[:, 1] - q1 * n[:, 0]
    rows = torch.stack([c0, c1, c2, n[:, 0], n[:, 1], n[:, 2]], dim=1)
    matched = live & valid & (n != 0).any(dim=1, keepdim=True) & (d2 <= _tol2(a["tol"]))[:, None]
    if a["normals"] is not None and a["has_cos"]:
        f = a["normals"]
        rot = [(t[k][0] * f[:, 0] + t[k][1] * f[:, 1]) + t[k][2] * f[:, 2] for k in range(3)]
        cosv = (rot[0] * n[:, 0] + rot[1] * n[:, 1]) + rot[2] * n[:, 2]
        matched = matched & (cosv >= a["cos"])[:, None]
    matched = matched & torch.isfinite(r)[:, None] & torch.isfinite(rows).all(dim=1, keepdim=True)
    return matched, r[:, None], rows, w


def _compose_system(a, T):
    """-> system fp64 [B,32] by torch.sum, and the per-pixel outputs zeroed where unmatched"""
    B, dev = a["B"], a["dev"]
    matched, r, rows, w = _compose_rows(a, T)
    zero = torch.zeros((), device=dev, dtype=torch.float32)
    r = torch.where(matched, r, zero)
    rows = torch.where(matched, rows, zero)
    md = matched.reshape(B, -1)
    g = rows.reshape(B, 6, -1).double()
    rd = r.reshape(B, -1).double()
    wd = torch.ones_like(rd) if w is None else w.reshape(B, -1).double()
    zd = torch.zeros((), device=dev, dtype=torch.float64)
    gw = wd[:, None] * g
    S = torch.zeros((B, SLOTS), device=dev, dtype=torch.float64)
    for k, (i, j) in enumerate(_TRI):
        S[:, k] = torch.where(md, gw[:, i] * g[:, j], zd).sum(dim=1)
    for i in range(6):
        S[:, 21 + i] = torch.where(md, gw[:, i] * rd, zd).sum(dim=1)
    S[:, 27] = torch.where(md, (wd * rd) * rd, zd).sum(dim=1)
    S[:, 28] = torch.where(md, wd, zd).sum(dim=1)
    S[:, 29] = md.sum(dim=1).double()
    return S, matched, r, rows


def _solve_restated(S, T, damping, min_count):
    """ud_icp_solve (csrc/icp_point.h) operation by operation on fp64 tensors [B]: -> (T_new fp32 [B,3,4], x fp64 [B,6], status bool [B])"""
    A = [[None] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(_TRI):
        A[i][j] = A[j][i] = S[:, k]
    for i in range(6):
        A[i][i] = A[i][i] + damping

    def dot(terms):
        s = None
        for term in terms:
            s = term if s is None else s + term
        return s

    L = [[None] * 6 for _ in range(6)]
    d, ok = [], S[:, 29] >= float(min_count)
    for j in range(6):
        d.append(A[j][j] if j == 0 else A[j][j] - dot((L[j][c] * L[j][c]) * d[c] for c in range(j)))
        ok = ok & (d[j] > 0)
        for i in range(j + 1, 6):
            L[i][j] = (A[i][j] if j == 0 else A[i][j] - dot((L[i][c] * L[j][c]) * d[c] for c in range(j))) / d[j]
    y = []
    for i in range(6):
        y.append(S[:, 21 + i] if i == 0 else S[:, 21 + i] - dot(L[i][c] * y[c] for c in range(i)))
    z = [y[i] / d[i] for i in range(6)]
    x = [None] * 6
    for i in range(5, -1, -1):
        x[i] = z[i] if i == 5 else z[i] - dot(L[c][i] * x[c] for c in range(i + 1, 6))
    for i in range(6):
        ok = ok & torch.isfinite(x[i])
    a0, a1, a2 = x[0] * 0.5, x[1] * 0.5, x[2] * 0.5
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    den, kk, t0, t1, t2 = 1.0 + aa, 1.0 - aa, 2.0 * a0, 2.0 * a1, 2.0 * a2
    R = [[(kk + t0 * a0) / den, (t0 * a1 - t2) / den, (t0 * a2 + t1) / den],
         [(t1 * a0 + t2) / den, (kk + t1 * a1) / den, (t1 * a2 - t0) / den],
         [(t2 * a0 - t1) / den, (t2 * a1 + t0) / den, (kk + t2 * a2) / den]]
    O = T.double()
    N = [[(R[i][0] * O[:, 0, j] + R[i][1] * O[:, 1, j]) + R[i][2] * O[:, 2, j] for j in range(4)] for i in range(3)]
    for i in range(3):
        N[i][3] = N[i][3] + x[3 + i]
    Tn = torch.stack([torch.stack(row, dim=-1) for row in N], dim=-2).float()
    Tn = torch.where(ok[:, None, None], Tn, T)
    xs = torch.where(ok[:, None], torch.stack(x, dim=-1), torch.zeros((), device=S.device, dtype=torch.float64))
    return Tn, xs, ok


def _rows_result(a, S, matched, r, rows, return_rows):
    if not return_rows:
        return S
    B, H, W = a["B"], a["H"], a["W"]
    return S, matched.view(B, 1, H, W), r.view(B, 1, H, W), rows.view(B, 6, H, W)


def icp_linearize_composition(frame: torch.Tensor, camera, model_points: torch.Tensor, model_normals: torch.Tensor, model_valid: torch.Tensor,
                              model_camera, transform: torch.Tensor, *, dist_tol: float, cos_tol: Optional[float] = None,
                              normals: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                              weights: Optional[torch.Tensor] = None, return_rows: bool = False):
    """icp_linearize's definition spelled with the separate calls: arguments and results as there, any of the six camera models on either
    side.  The point comes from gt_points(frame, camera) (or is the given point map); the move is spelled element-wise in ud_cam_move's
    association, x' = ((t00 x + t01 y) + t02 z) + t03; project_camera(q, model_camera, (Hm, Wm)) gives (u, v), inside and the depth of q;
    remap(cat(model_points, model_normals), uv, mode="nearest", coord_valid=inside & (depth > 0), src_mask=model_valid, return_mask=True)
    the model's point and normal and the validity of the model pixel; torch element-wise arithmetic, every operation a launch of its own,
    forms the residual, the row and the decision; the 30 sums are torch.sum in fp64 over (w g_i) g_j and the other terms of the fused form.
    The per-pixel outputs have the fused kernel's bits; the sums differ from it by the order of summation only."""
    a = _arguments("icp_linearize_composition", frame, camera, model_points, model_normals, model_valid, model_camera, transform, dist_tol,
                   cos_tol, normals, mask, weights)
    with torch.cuda.device(a["dev"]):
        S, matched, r, rows = _compose_system(a, a["T"])
    return _rows_result(a, S, matched, r, rows, return_rows)


# ---- the fused form ------------------------------------------------------------------------------------------------------------------

def _frame_points(a):
    """an OPENCV / Fisheye624 frame camera with a depth: its points come from gt_points first (the radial loop ends on a maximum over the
    whole image), the route warp_camera takes"""
    if a["points"] is None and _args.n_iterative(a["cam"]):
        a["points"], a["depth"] = gt_points(a["depth"], a["cam"]), None


def _work(a):
    nbytes = int(_lib.lib.ud_icp_workspace_bytes(a["B"], a["H"], a["W"]))
    return torch.empty(nbytes // 8, device=a["dev"], dtype=torch.float64), nbytes


def _desc(a, T, work, nbytes, system, **kw):
    depth_form = a["points"] is None
    desc = mk(_lib.UdIcp, depth=a["depth"], points=a["points"], params=a["cam"].params if depth_form else None, mask=a["mask"],
              weights=a["weights"], normals=a["normals"], model_points=a["mp"], model_normals=a["mn"], model_valid=a["mv"],
              params_model=a["mcam"].params, T=T, work=work, system=system, work_bytes=nbytes, B=a["B"], H=a["H"], W=a["W"], Hm=a["Hm"],
              Wm=a["Wm"], nT=T.shape[0], has_cos=int(a["has_cos"]), dist_tol_bits=a["tol_bits"], cos_tol_bits=a["cos_bits"], **_LAUNCH_OPTIONS, **kw)
    if depth_form:
        _args.set_models(desc.model_frame, a["cam"])
    _args.set_models(desc.model_model, a["mcam"])
    return desc


def icp_linearize(frame: torch.Tensor, camera, model_points: torch.Tensor, model_normals: torch.Tensor, model_valid: torch.Tensor, model_camera,
                  transform: torch.Tensor, *, dist_tol: float, cos_tol: Optional[float] = None, normals: Optional[torch.Tensor] = None,
                  mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, return_rows: bool = False):
    """The normal system of one point-to-plane Gauss-Newton step of a frame against a model view, the whole batch in two launches.

    frame          the frame's depth [B,1,H,W] / [B,H,W] with its camera, or its point map [B,3,H,W] in the frame camera's coordinates
                   (camera is ignored then and may be None).  Any float dtype, converted to contiguous fp32.
    camera         as gtpoints.prepare_camera takes it for B images; a PreparedCamera is accepted and nothing is copied from the host then.
                   With an OPENCV or Fisheye624 member the points come from gt_points first (more launches).
    model_points, model_normals, model_valid     [B,3,Hm,Wm], [B,3,Hm,Wm] and bool / uint8 [B,1,Hm,Wm] / [B,Hm,Wm], in the model camera's
                   frame: what tsdf_render(..., return_points=True, return_normals=True) returns.
    model_camera   the camera of the model maps, any of the six models; only its projection is used.
    transform      fp32 [3,4] / [4,4] (or [1,..] / [B,..]): the current estimate, FRAME CAMERA TO MODEL CAMERA coordinates.
    dist_tol       a match needs |m - q| <= dist_tol, in the maps' units, rounded to fp32.
    cos_tol, normals   with both, a match needs (R nf) . n >= cos_tol, nf the frame's normals [B,3,H,W]; cos_tol in -1 .. 1.
    mask           bool / uint8 [B,1,H,W] / [B,H,W]: frame pixels with 0 are not used.
    weights        [B,1,H,W] / [B,H,W], any float dtype: the weight of each pixel's residual, for example infer()'s confidence; 1 without.
                   A pixel whose weight is not a finite positive number is not used.

    Frame pixel (x, y): p = the camera's reconstruct at the pixel centre (or the given point); live = depth > 0 (points: all finite) &
    mask & weight ok; q = T p; (u, v) = model_camera's projection of q; usable = its in-image test & depth of q > 0 & finite; m, n = the
    model maps at the nearest pixel where model_valid (remap's mode="nearest" and `valid`); e = m - q, d2 = (e0 e0 + e1 e1) + e2 e2,
    r = (n0 e0 + n1 e1) + n2 e2, c = q x n, all in fp32.  matched = live & usable & the model pixel valid & n != 0 & d2 <= dist_tol^2 &
    the normal test & everything finite -- false whenever a NaN is compared.  The row is g = (c, n).

    ->  system fp64 [B,32]: sum over the matched pixels of w g_i g_j for i <= j (21 values, the upper triangle of A row-major), w g_i r (6,
        b), w r r (e), w (wsum), 1 (count, exact), two zeros.  The update x = (omega, v) that minimises sum w (r - g . x)^2 solves A x = b
        (icp_solve).  Summed in a fixed order: bit-identical from call to call.
        With return_rows=True also matched bool [B,1,H,W], residual fp32 [B,1,H,W], rows fp32 [B,6,H,W], each exactly 0 where not matched.

    Two launches (csrc/icp.hip: the rows with the workgroups' partial sums, then their sum per image), no atomics.  Stream-ordered,
    nothing synchronises: captures into a graph (with PreparedCamera cameras).  The HIP kernels are the only implementation: CPU tensors
    raise."""
    fn = "icp_linearize"
    a = _arguments(fn, frame, camera, model_points, model_normals, model_valid, model_camera, transform, dist_tol, cos_tol, normals, mask, weights)
    B, H, W, dev = a["B"], a["H"], a["W"], a["dev"]
    with torch.cuda.device(dev):
        _frame_points(a)
        work, nbytes = _work(a)
        system = torch.empty((B, SLOTS), device=dev, dtype=torch.float64)
        matched = torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8) if return_rows else None
        residual = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32) if return_rows else None
        rows = torch.empty((B, 6, H, W), device=dev, dtype=torch.float32) if return_rows else None
        desc = _desc(a, a["T"], work, nbytes, system, matched=matched, residual=residual, rows=rows, solve=0)
        check(_lib.lib.ud_icp_linearize(desc, cur_stream()), "ud_icp_linearize")
    return _rows_result(a, system, matched.view(torch.bool) if return_rows else None, residual, rows, return_rows)


def icp_solve(system: torch.Tensor, transform: torch.Tensor, *, damping: float = 0.0, min_count: int = 6):
    """The update of icp_linearize's system and the new estimate: (A + damping I) x = b by LDL^T without pivoting in fp64, using + - * /
    only, in the order fixed in csrc/icp_point.h; status = count >= min_count, every pivot > 0 and x finite.  With x = (omega, v) and
    a = omega / 2 the rotation is the Cayley map R = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), and T_new = [R R_old | R t_old + v],
    formed in fp64 from the widened fp32 transform and rounded to fp32 once.

    system fp64 [B,32] on the GPU; transform fp32 [3,4] / [4,4] (or [1,..] / [B,..]), not modified.
    ->  (T_new fp32 [B,3,4], x fp64 [B,6], status bool [B]); where status is False T_new is the transform as it was and x is 0.
    One launch (ud_icp_update), nothing synchronises."""
    fn = "icp_solve"
    if not isinstance(system, torch.Tensor) or system.dtype != torch.float64 or system.ndim != 2 or system.shape[1] != SLOTS or system.shape[0] == 0:
        raise ValueError(f"{fn}: system must be fp64 [B,{SLOTS}], non-empty")
    B = system.shape[0]
    _args.max_images(fn, B)
    if transform is None:
        raise ValueError(f"{fn}: transform must be fp32 [3,4], [4,4], [1,..] or [{B},..]")
    T, _ = _args.rigid(fn, transform, B)
    dm = _damping(fn, damping, min_count)
    dev = system.device
    _args.one_gpu(fn, dev, T)
    with torch.cuda.device(dev):
        Tn = T.expand(B, 3, 4).clone()
        x = torch.empty((B, 6), device=dev, dtype=torch.float64)
        status = torch.empty((B,), device=dev, dtype=torch.uint8)
        desc = mk(_lib.UdIcp, system=system.contiguous(), T=Tn, x=x, status=status, B=B, nT=B, solve=1, min_count=min_count,
                  damping_bits=_f64_bits(dm))
        check(_lib.lib.ud_icp_update(desc, cur_stream()), "ud_icp_update")
    return Tn, x, status.view(torch.bool)


def _start(a, transform):
    B, dev = a["B"], a["dev"]
    if transform is None:
        return torch.eye(4, device=dev, dtype=torch.float32)[:3].expand(B, 3, 4).clone()
    return a["T"].expand(B, 3, 4).clone()


def track_camera(frame: torch.Tensor, camera, model_points: torch.Tensor, model_normals: torch.Tensor, model_valid: torch.Tensor, model_camera,
                 transform: Optional[torch.Tensor] = None, *, iters: int = 10, dist_tol: float, cos_tol: Optional[float] = None,
                 normals: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                 damping: float = 0.0, min_count: int = 6):
    """A frame aligned to a model view by `iters` Gauss-Newton steps of projective point-to-plane ICP: icp_linearize and icp_solve `iters`
    times on one T buffer, two launches per step.  Arguments as icp_linearize and icp_solve; transform is the starting estimate, FRAME
    CAMERA TO MODEL CAMERA coordinates, None: the identity.

    ->  (T fp32 [B,3,4], stats fp64 [B,iters,4]): the estimate after the last step, and per step e = sum w r^2, wsum, the matched count
        and the status, all taken at the estimate the step started from.  A step whose status is 0 leaves T as it was; the steps after it
        still run.

    Stream-ordered with no host synchronisation, 2 * iters launches and no other work between them (an OPENCV / Fisheye624 frame camera
    adds gt_points' launches once); captures into a graph when the cameras are PreparedCameras.  The HIP kernels are the only
    implementation: CPU tensors raise."""
    fn = "track_camera"
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= 1000:
        raise ValueError(f"{fn}: iters must be an integer in 1 .. 1000, got {iters!r}")
    dm = _damping(fn, damping, min_count)
    a = _arguments(fn, frame, camera, model_points, model_normals, model_valid, model_camera, transform, dist_tol, cos_tol, normals, mask, weights,
                   need_T=False)
    B, dev = a["B"], a["dev"]
    with torch.cuda.device(dev):
        _frame_points(a)
        T = _start(a, transform)
        work, nbytes = _work(a)
        system = torch.empty((B, SLOTS), device=dev, dtype=torch.float64)
        stats = torch.empty((B, iters, 4), device=dev, dtype=torch.float64)
        desc = _desc(a, T, work, nbytes, system, solve=1, min_count=min_count, damping_bits=_f64_bits(dm), stats_stride=iters * 4)
        stream = cur_stream()
        for it in range(iters):
            desc.stats = stats.data_ptr() + it * 4 * 8
            check(_lib.lib.ud_icp_linearize(desc, stream), "ud_icp_linearize")
    return T, stats


def track_camera_composition(frame: torch.Tensor, camera, model_points: torch.Tensor, model_normals: torch.Tensor, model_valid: torch.Tensor,
                             model_camera, transform: Optional[torch.Tensor] = None, *, iters: int = 10, dist_tol: float,
                             cos_tol: Optional[float] = None, normals: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                             weights: Optional[torch.Tensor] = None, damping: float = 0.0, min_count: int = 6):
    """track_camera's definition spelled with the separate calls: arguments and results as there.  Per step icp_linearize_composition's
    launches (gt_points once, then project_camera, remap and about 60 element-wise ones, 30 torch.sum in fp64) and ud_icp_solve restated
    in torch fp64 on [B] tensors, operation by operation in the order of csrc/icp_point.h (about 400 launches).  Nothing synchronises.
    This is the oracle of the fused kernels' tests and the counterpart of their benchmark."""
    fn = "track_camera_composition"
    if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= 1000:
        raise ValueError(f"{fn}: iters must be an integer in 1 .. 1000, got {iters!r}")
    dm = _damping(fn, damping, min_count)
    a = _arguments(fn, frame, camera, model_points, model_normals, model_valid, model_camera, transform, dist_tol, cos_tol, normals, mask, weights,
                   need_T=False)
    with torch.cuda.device(a["dev"]):
        if a["points"] is None:
            a["points"], live = gt_points(a["depth"], a["cam"]), a["depth"] > 0
            # the liveness of the depth form (depth > 0) enters through the mask; the points are computed once for all steps
            a["mask"] = live.view(torch.uint8) if a["mask"] is None else (live & a["mask"].bool()).view(torch.uint8)
            a["depth"] = None
        T = _start(a, transform)
        stats = []
        for _ in range(iters):
            S = _compose_system(a, T)[0]
            T, _, ok = _solve_restated(S, T, dm, min_count)
            stats.append(torch.stack([S[:, 27], S[:, 28], S[:, 29], ok.double()], dim=-1))
    return T, torch.stack(stats, dim=1)
