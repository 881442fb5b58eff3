"""The conditioning of a depth frame and coarse-to-fine tracking: the two stages of a KinectFusion-style front end between infer() and
track_camera.

    prepare_depth_filter(radius, sigma_space, sigma_range, device)     the bilateral filter's two tables, uploaded once
    depth_pyramid(depth, levels, ...)          the filtered frame and its gated 2 x 2 means, every level in ONE launch: ud_depth_pyramid
                                               (csrc/pyramid.hip; the arithmetic of a pixel is csrc/pyramid_point.h)
    depth_pyramid_composition(...)             the same definition in vectorised torch, shifted slices in the same accumulation order
    pyramid_cameras(camera, B, levels, device) the camera of every level, finest first, for all six models
    track_camera_pyramid(depth, camera, model_levels, ...)    one depth_pyramid launch, then icp.track_camera's steps level by level,
                                               coarsest first, on one T buffer
    TsdfVolume.track_pyramid(...)              the volume rendered once per level, then track_camera_pyramid (tsdf.py)

A pixel is live when mask != 0 and 0 < depth < +inf (with weights: and 0 < w < +inf); a pixel that is not live is 0 at every level, the
chain's "no depth".  Every operation is one separately rounded fp32 operation in a fixed order, so a numpy restatement reproduces every
bit.  The HIP kernel is the only implementation of the fused form: CPU tensors raise."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _args, _lib, icp
from .cameras import GT_SPHERICAL
from .gtpoints import PreparedCamera, prepare_camera
from .normals import normals_camera
from .ops import check, cur_stream, mk

NB = 256                   # UD_PY_NB: bins of the range table
MAX_RADIUS, MAX_LEVELS = 4, 4
# how ud_depth_pyramid runs: the level-0 tile of a workgroup (0: the default, 1: 32 x 32, 2: 64 x 16).  The result does not depend on it;
# tools/bench_pyramid.py measures both (profiles/pyramid_bench.txt).
_LAUNCH_OPTIONS = dict(tile=0)


class DepthFilter:
    """prepare_depth_filter's result: radius, ws fp32 [(2r+1)^2] and wr fp32 [256] on the device, and the bit pattern of inv_bin"""

    def __init__(self, radius: int, ws: torch.Tensor, wr: torch.Tensor, inv_bin_bits: int):
        self.radius, self.ws, self.wr, self.inv_bin_bits = radius, ws, wr, inv_bin_bits


def filter_tables(radius: int, sigma_space: float, sigma_range: float):
    """-> (ws fp32 [(2r+1)^2], wr fp32 [256], inv_bin fp32) as numpy, built in fp64 and rounded to fp32 once:
    ws = exp(-(dx^2 + dy^2) / (2 sigma_space^2)), dy outer; wr[k] = exp(-((k + 0.5) bin)^2 / (2 sigma_range^2)) with bin = 3 sigma_range /
    256 and wr[255] = 0 (everything beyond 3 sigma_range is rejected); inv_bin = 1 / bin."""
    fn = "prepare_depth_filter"
    _args.radius(fn, radius, MAX_RADIUS)
    ss, sr = _args.positive(fn, "sigma_space", sigma_space), _args.positive(fn, "sigma_range", sigma_range)
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        ws = np.exp(-(ax[None, :] ** 2 + ax[:, None] ** 2) / (2.0 * ss * ss)).reshape(-1).astype(np.float32)
        step = 3.0 * sr / NB
        wr = np.exp(-(((np.arange(NB, dtype=np.float64) + 0.5) * step) ** 2) / (2.0 * sr * sr)).astype(np.float32)
        wr[NB - 1] = 0.0
        inv_bin = np.float32(1.0 / step)
    if not (ws[len(ws) // 2] > 0 and wr[0] > 0 and np.isfinite(inv_bin) and inv_bin > 0):
        raise ValueError(f"{fn}: sigma_space={sigma_space} sigma_range={sigma_range} give a table whose centre weight, first range weight "
                         f"or bin width is not a positive fp32 number")
    return ws, wr, inv_bin


def prepare_depth_filter(radius: int, sigma_space: float, sigma_range: float, device) -> DepthFilter:
    """The bilateral filter of depth_pyramid's level 0: radius 0 .. 4 pixels, sigma_space in pixels, sigma_range in the depth's units.
    The two tables (filter_tables) are built on the host and uploaded once: call it outside a graph capture, as prepare_camera."""
    ws, wr, inv_bin = filter_tables(radius, sigma_space, sigma_range)
    _args.one_gpu("prepare_depth_filter", torch.device(device))
    return DepthFilter(radius, torch.from_numpy(ws).to(device), torch.from_numpy(wr).to(device), _args.f32_bits(float(inv_bin)))


def _arguments(fn, depth, levels, mask, weights, filter, gate):
    B, H, W = _args.depth_map(fn, "depth", depth)
    _args.max_images(fn, B)
    _args.levels(fn, levels, H, W, MAX_LEVELS)
    _args.max_elems(fn, f"H={H} W={W}", H * W)
    if H > 16 * 65535:                                                # the launch grid's rows of tiles
        raise ValueError(f"{fn}: unsupported sizes H={H} W={W}")
    if mask is not None:
        _args.image_map(fn, "mask", mask, H, W, mask=True, B=B, shared=False)
    if weights is not None:
        _args.image_map(fn, "weights", weights, H, W, mask=False, B=B, shared=False)
    if filter is not None and not isinstance(filter, DepthFilter):
        raise ValueError(f"{fn}: filter must be a prepare_depth_filter() result or None, got {type(filter).__name__}")
    gate_bits = _args.gate(fn, "gate", gate)
    dev = depth.device
    _args.one_gpu(fn, dev, mask, weights, *((filter.ws, filter.wr) if filter is not None else ()))
    with torch.cuda.device(dev):
        d = depth.reshape(B, 1, H, W).float().contiguous()
        m = None if mask is None else mask.reshape(B, 1, H, W).contiguous().view(torch.uint8)
        w = None if weights is None else weights.reshape(B, 1, H, W).float().contiguous()
    return dict(B=B, H=H, W=W, L=levels, dev=dev, depth=d, mask=m, weights=w, filter=filter, gate_bits=gate_bits,
                sizes=[(H >> l, W >> l) for l in range(levels)])


def _launch(a):
    B, dev, f = a["B"], a["dev"], a["filter"]
    with torch.cuda.device(dev):
        out_d = [torch.empty((B, 1, h, w), device=dev, dtype=torch.float32) for h, w in a["sizes"]]
        out_w = [torch.empty((B, 1, h, w), device=dev, dtype=torch.float32) for h, w in a["sizes"]] if a["weights"] is not None else None
        desc = mk(_lib.UdDepthPyramid, depth=a["depth"], mask=a["mask"], weights=a["weights"], ws=None if f is None else f.ws,
                  wr=None if f is None else f.wr, B=B, H=a["H"], W=a["W"], levels=a["L"], radius=0 if f is None else f.radius,
                  gate_bits=a["gate_bits"], inv_bin_bits=0 if f is None else f.inv_bin_bits, **_LAUNCH_OPTIONS)
        for l in range(a["L"]):
            desc.out_depth[l] = out_d[l].data_ptr()
            if out_w is not None:
                desc.out_weights[l] = out_w[l].data_ptr()
        check(_lib.lib.ud_depth_pyramid(desc, cur_stream()), "ud_depth_pyramid")
    return out_d, out_w


def depth_pyramid(depth: torch.Tensor, levels: int = 3, *, mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                  filter: Optional[DepthFilter] = None, gate: float = math.inf):
    """A depth frame conditioned for tracking: the bilateral filter at level 0 and `levels` - 1 gated halvings, the batch in ONE launch.

    depth     [B,1,H,W] / [B,H,W], any float dtype (converted to contiguous fp32); H, W >= 2^(levels - 1); 1 <= levels <= 4.
    mask      bool / uint8 [B,1,H,W] / [B,H,W]: pixels with 0 are not live.
    weights   [B,1,H,W] / [B,H,W], any float dtype, for example infer()'s confidence: a pixel whose weight is not a finite positive number
              is not live; with weights a weight map is returned for every level.
    filter    a prepare_depth_filter() result; None: radius 0, level 0 is the live depths.
    gate      a 2 x 2 block of a coarser level averages the members within `gate` of its NEAREST live member (fp32, >= 0, inf: all),
              so a block on a depth edge never becomes a phantom depth between two surfaces.

    Level 0: for a live centre dc and every live tap d inside the image, dy = -r..r (outer), dx = -r..r (inner): delta = |d - dc|,
    bin = 255 where delta * inv_bin >= 256 else int(delta * inv_bin), w = ws[dy, dx] * wr[bin], num += w d, den += w; out = num / den.
    Level l: H_l = H_{l-1} // 2, W_l = W_{l-1} // 2; the members (2y,2x), (2y,2x+1), (2y+1,2x), (2y+1,2x+1) are live where > 0; the
    included ones are summed in that order and divided by their count, their weights likewise by the same count.  The weight of level 0
    is the pixel's own where live.  Everything is 0 where nothing is live (csrc/pyramid_point.h has the definition operation by operation).

    ->  [depth_0, ..., depth_{L-1}], fp32 [B,1,H_l,W_l]; with weights ([depth_l], [weights_l]).
    One launch, stream-ordered, nothing synchronises, no workspace: captures into a graph."""
    a = _arguments("depth_pyramid", depth, levels, mask, weights, filter, gate)
    out_d, out_w = _launch(a)
    return out_d if out_w is None else (out_d, out_w)


def depth_pyramid_composition(depth: torch.Tensor, levels: int = 3, *, mask: Optional[torch.Tensor] = None,
                              weights: Optional[torch.Tensor] = None, filter: Optional[DepthFilter] = None, gate: float = math.inf):
    """depth_pyramid's definition in vectorised torch: arguments and results as there.  The taps are shifted slices of the zero-padded
    staged map, accumulated with torch.where in the kernel's tap order; a level is four strided slices of the one before.  Every
    element-wise operation is a launch of its own and rounds once, so the results have the fused kernel's bits: the second oracle of its
    tests and the counterpart of its benchmark."""
    a = _arguments("depth_pyramid_composition", depth, levels, mask, weights, filter, gate)
    dev, H, W, f = a["dev"], a["H"], a["W"], a["filter"]
    with torch.cuda.device(dev):
        d, w = a["depth"], a["weights"]
        zero = torch.zeros((), device=dev, dtype=torch.float32)
        live = (d > 0) & (d <= torch.finfo(torch.float32).max)
        if a["mask"] is not None:
            live = live & (a["mask"] != 0)
        if w is not None:
            live = live & (w > 0) & (w <= torch.finfo(torch.float32).max)
        staged = torch.where(live, d, zero)
        r = 0 if f is None else f.radius
        if r == 0:
            level = staged
        else:
            inv_bin = filter_inv_bin(f)                                    # a Python float that holds the fp32 exactly
            padded = torch.nn.functional.pad(staged, (r, r, r, r))
            num, den = torch.zeros_like(staged), torch.zeros_like(staged)
            k = 2 * r + 1
            for dy in range(k):
                for dx in range(k):
                    t = padded[:, :, dy:dy + H, dx:dx + W]
                    used = t > 0
                    q = (t - staged).abs() * inv_bin
                    idx = torch.where(q >= float(NB), torch.full_like(q, NB - 1), q).long()
                    wt = f.ws[dy * k + dx] * f.wr[idx]
                    num = torch.where(used, num + wt * t, num)
                    den = torch.where(used, den + wt, den)
            level = torch.where(live, num / den, zero)
        out_d, out_w = [level], None if w is None else [torch.where(live, w, zero)]
        gate_v = float(np.array([a["gate_bits"]], np.int32).view(np.float32)[0])
        for l in range(1, a["L"]):
            h, wd = a["sizes"][l]
            prev = out_d[-1]
            mem = [prev[:, :, i:2 * h:2, j:2 * wd:2] for i in (0, 1) for j in (0, 1)]
            any_live, anchor = torch.zeros_like(mem[0], dtype=torch.bool), torch.zeros_like(mem[0])
            for m in mem:
                lv = m > 0
                anchor = torch.where(lv & (~any_live | (m < anchor)), m, anchor)
                any_live = any_live | lv
            inc = [(m > 0) & (m - anchor <= gate_v) for m in mem]
            n = torch.zeros_like(mem[0])
            total = torch.zeros_like(mem[0])
            for m, i in zip(mem, inc):
                total = torch.where(i, torch.where(n > 0, total + m, m), total)
                n = n + i.float()
            out_d.append(torch.where(n > 0, total / n, zero))
            if out_w is not None:
                pw = out_w[-1]
                wm = [pw[:, :, i:2 * h:2, j:2 * wd:2] for i in (0, 1) for j in (0, 1)]
                k, wt = torch.zeros_like(mem[0]), torch.zeros_like(mem[0])
                for m, i in zip(wm, inc):
                    wt = torch.where(i, torch.where(k > 0, wt + m, m), wt)
                    k = k + i.float()
                out_w.append(torch.where(n > 0, wt / n, zero))
    return out_d if out_w is None else (out_d, out_w)


def filter_inv_bin(f: DepthFilter) -> float:
    """the fp32 inv_bin of a filter as a Python float"""
    return float(np.array([f.inv_bin_bits], np.int32).view(np.float32)[0])


def pyramid_cameras(camera, B: int, levels: int, device) -> list:
    """The camera of every pyramid level as PreparedCameras, finest first.  Level l is DEFINED by project_l(P) == project_0(P) / 2^l and
    unproject_l(uv) == unproject_0(2^l uv): with pixel centres at half-integers the block (2x, 2x + 1) sits at x + 0.5.  For Pinhole,
    EUCM, OPENCV, Fisheye624 and MEI that is the columns fx, fy, cx, cy times 2^-l.  Spherical maps through (W - 1) and (H - 1)
    (csrc/camera_models.h: u = lon / (2 hfov) * (W - 1) + (W - 1) / 2), so its W and H columns become (p + 1) / 2 per level: then
    (p' - 1) = (p - 1) / 2.  All of it is exact in fp32 (powers of two; integer sizes below 2^23).  camera: as prepare_camera takes
    it.  The multipliers are built from the model tags with device-side fills and applied on the device: nothing is read back, and with a
    PreparedCamera nothing is copied from the host (graph capture)."""
    fn = "pyramid_cameras"
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"{fn}: levels must be an integer in 1 .. {MAX_LEVELS}, got {levels!r}")
    cam = prepare_camera(camera, B, device)
    _args.one_gpu(fn, cam.params.device)
    with torch.cuda.device(cam.params.device):
        return [PreparedCamera(rows, cam.models) for rows in level_rows(cam.params, cam.models, levels)]


def level_rows(rows: torch.Tensor, models, levels: int) -> list:
    """pyramid_cameras' arithmetic on parameter rows fp32 [B,16] (any device) with the model tag of every row: -> the rows of every level,
    finest first.  One step is rows * mul + add: mul 0.5 in columns 0..3 of every row, mul 0.5 and add 0.5 in columns 4, 5 of a
    Spherical row, mul 1 and add 0 elsewhere; level l is l steps."""
    B = rows.shape[0]
    out = [rows]
    if levels == 1:
        return out
    mul = torch.ones((B, 16), device=rows.device, dtype=torch.float32)
    add = torch.zeros((B, 16), device=rows.device, dtype=torch.float32)
    mul[:, 0:4] = 0.5
    b = 0
    while b < B:                                                       # one fill per run of Spherical rows
        if models[b] != GT_SPHERICAL:
            b += 1
            continue
        e = b
        while e < B and models[e] == GT_SPHERICAL:
            e += 1
        mul[b:e, 4:6] = 0.5
        add[b:e, 4:6] = 0.5
        b = e
    for _ in range(1, levels):
        rows = rows * mul + add
        out.append(rows)
    return out


def _iters(fn, iters, L):
    try:
        its = tuple(iters)
    except TypeError:
        raise ValueError(f"{fn}: iters must be a sequence of {L} integers, finest level first") from None
    if len(its) != L or any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i <= 1000 for i in its) or sum(its) < 1:
        raise ValueError(f"{fn}: iters must be {L} integers in 0 .. 1000, finest level first, not all 0, got {iters!r}")
    return its


def _level_cameras(fn, camera, B, L, dev):
    if isinstance(camera, (list, tuple)) and len(camera) > 0 and all(isinstance(c, PreparedCamera) for c in camera):
        if len(camera) != L:
            raise ValueError(f"{fn}: {len(camera)} level cameras for {L} levels")
        return list(camera)
    if camera is None:
        raise ValueError(f"{fn}: camera is required")
    return pyramid_cameras(camera, B, L, dev)


def track_camera_pyramid(depth: torch.Tensor, camera, model_levels: Sequence, transform: Optional[torch.Tensor] = None, *, dist_tol: float,
                         iters: Sequence[int] = (10, 5, 4), filter: Optional[DepthFilter] = None, gate: float = math.inf,
                         cos_tol: Optional[float] = None, mask: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                         damping: float = 0.0, min_count: int = 6):
    """Coarse-to-fine track_camera: one depth_pyramid launch, then per level, coarsest first, iters[l] steps of icp.track_camera on one T
    buffer with that level's depth, weights and camera.

    depth         the frame's depth [B,1,H,W] / [B,H,W]; a point map raises ValueError (a pyramid needs the camera of every level).
    camera        as prepare_camera takes it (level l through pyramid_cameras), or a pyramid_cameras() list of len(model_levels).
    model_levels  L tuples (model_points, model_normals, model_valid, model_camera), finest first, each with its own size and camera:
                  what tsdf_render gives at size >> l through pyramid_cameras(...)[l].
    iters         L integers, FINEST FIRST, executed coarsest first; 0 skips its level.
    filter, gate, mask, weights     depth_pyramid's; the mask and the weights' liveness are folded into the pyramid (a dead pixel has
                  depth 0), the weights of every level are that level's weight map.
    cos_tol       with it, every level's frame normals come from normals_camera(depth_l, camera_l).
    transform, dist_tol, damping, min_count    track_camera's.

    ->  (T fp32 [B,3,4], stats fp64 [B,sum(iters),4]) in execution order.  It is BY DEFINITION the chain depth_pyramid, pyramid_cameras
        and track_camera level by level, bit for bit.  1 + 2 sum(iters) launches, plus one per used level with cos_tol (and gt_points'
        for an OPENCV / Fisheye624 frame camera); nothing synchronises: captures into a graph with prepared cameras."""
    fn = "track_camera_pyramid"
    _args.float_tensor(fn, "depth", depth)
    if depth.ndim == 4 and depth.shape[1] == 3:
        raise ValueError(f"{fn}: a [B,3,H,W] point map cannot be tracked through a pyramid; pass the depth and its camera")
    try:
        model_levels = [tuple(m) for m in model_levels]
    except TypeError:
        raise ValueError(f"{fn}: model_levels must be a sequence of (points, normals, valid, camera) tuples, finest first") from None
    L = len(model_levels)
    if not 1 <= L <= MAX_LEVELS or any(len(m) != 4 for m in model_levels):
        raise ValueError(f"{fn}: model_levels must be 1 .. {MAX_LEVELS} tuples (points, normals, valid, camera), finest first")
    its = _iters(fn, iters, L)
    dm = icp._damping(fn, damping, min_count)
    a = _arguments(fn, depth, L, mask, weights, filter, gate)
    B, dev = a["B"], a["dev"]
    cams = _level_cameras(fn, camera, B, L, dev)
    T0, _ = _args.rigid(fn, transform, B)
    _args.one_gpu(fn, dev, T0)
    total = sum(its)
    with torch.cuda.device(dev):
        out_d, out_w = _launch(a)
        T = torch.eye(4, device=dev, dtype=torch.float32)[:3].expand(B, 3, 4).clone() if T0 is None else T0.expand(B, 3, 4).clone()
        stats = torch.empty((B, total, 4), device=dev, dtype=torch.float64)
        stream, done = cur_stream(), 0
        for l in reversed(range(L)):
            if not its[l]:
                continue
            mp, mn, mv, mcam = model_levels[l]
            nl = normals_camera(out_d[l], cams[l]) if cos_tol is not None else None
            b = icp._arguments(fn, out_d[l], cams[l], mp, mn, mv, mcam, T, dist_tol, cos_tol, nl, None, None if out_w is None else out_w[l],
                               need_T=False)
            icp._frame_points(b)
            work, nbytes = icp._work(b)
            system = torch.empty((B, icp.SLOTS), device=dev, dtype=torch.float64)
            desc = icp._desc(b, T, work, nbytes, system, solve=1, min_count=min_count, damping_bits=icp._f64_bits(dm), stats_stride=total * 4)
            for it in range(its[l]):
                desc.stats = stats.data_ptr() + (done + it) * 4 * 8
                check(_lib.lib.ud_icp_linearize(desc, stream), "ud_icp_linearize")
            done += its[l]
    return T, stats
