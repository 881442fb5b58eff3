"""Host-side mirror of the reference's two native extensions (evaluation / loss side), over the C-ABI of include/unidepth_hip.h:

    knn_points, knn_gather          unidepth/ops/knn/functions/knn.py:113-196, 199-249  (forward; the KNN extension)
    ChamferDistance, chamfer_dist   unidepth/utils/chamfer_distance.py:60-159, unidepth/utils/evaluation_depth.py:12-18
    auc, f1_score, DICT_METRICS_3D, eval_3d   unidepth/utils/evaluation_depth.py:21-34,74-91,109-125,160-182 (the 3-D metrics)
    eval_depth, DICT_METRICS, DICT_METRICS_D  unidepth/utils/evaluation_depth.py:37-72,93-110,124-147 (the 2-D depth metrics)
    eval_3d_batch, eval_3d_size, thresholds_3d  eval_3d of a whole batch in one ud_eval_3d call (csrc/eval3d.hip), no host synchronisation
    MetricsAccumulator              datasets/base_dataset.py:219-271 (metrics_store / metrics_count / get_evaluation, one process)
    RandomPatchExtractor            unidepth/ops/extract_patches/modules/patch_extractor.py:10-42 (forward)

Same names, argument meaning and error behaviour; inference / evaluation only (no autograd: the reference's backward kernels are
training code).  Tensors must live on the GPU: there is no CPU path.  eval_depth / DICT_METRICS compute in fp32 whatever the input
dtype (the reference computes in the input dtype), and run in ud_eval_depth without any host synchronisation."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .ops import check, cur_stream, mk

_KNN = namedtuple("KNN", "dists idx knn")


def _lengths(lengths: Optional[torch.Tensor], N: int, device) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    if lengths.ndim != 1 or lengths.shape[0] != N:
        raise ValueError("Expected lengths to be of shape (N,)")
    return lengths.to(device=device, dtype=torch.int64).contiguous()


def knn_points(p1: torch.Tensor, p2: torch.Tensor, lengths1: Union[torch.Tensor, None] = None, lengths2: Union[torch.Tensor, None] = None,
               norm: int = 2, K: int = 1, version: int = -1, return_nn: bool = False, return_sorted: bool = True) -> _KNN:
    """K nearest neighbours in p2 of every point of p1 (functions/knn.py:113-196).  `version` selected a CUDA kernel variant in the
    reference and is accepted and ignored; the result is always sorted ascending (what return_sorted=True gives the reference; an
    unsorted result is any order, so this satisfies return_sorted=False too).  dists are squared L2 (norm 2) or L1 (norm 1)."""
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    if not p1.is_cuda or not p2.is_cuda:
        raise RuntimeError("knn_points: GPU tensors expected (the HIP kernel is the only implementation)")
    p1 = p1.float().contiguous()
    p2 = p2.float().contiguous()
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    l1 = _lengths(lengths1, N, p1.device)
    l2 = _lengths(lengths2, N, p1.device)
    dists = torch.empty(N, P1, K, device=p1.device, dtype=torch.float32)
    idx = torch.empty(N, P1, K, device=p1.device, dtype=torch.int64)
    if N * P1 * K:
        d = mk(_lib.UdKnn, p1=p1, p2=p2, lengths1=l1, lengths2=l2, dists=dists, idx=idx, work=None, N=N, P1=P1, P2=P2, D=D, K=K, norm=norm)
        if K == 1 and -(-P1 // 512) * N < 1024 and P2 > 4096:
            work = torch.empty(N * P1, device=p1.device, dtype=torch.int64)     # scratch for the P2-split merge
            d.work = work.data_ptr()
        check(_lib.lib.ud_knn_points(d, cur_stream()), "ud_knn_points")
    nn = knn_gather(p2, idx, lengths2) if return_nn else None
    return _KNN(dists=dists, idx=idx, knn=nn)


def knn_gather(x: torch.Tensor, idx: torch.Tensor, lengths: Union[torch.Tensor, None] = None) -> torch.Tensor:
    """x_out[n, l, k] = x[n, idx[n, l, k]] for features x [N, M, U] and neighbour indices idx [N, L, K]; slots k >= lengths[n] (clouds
    with fewer than K points) are zero (functions/knn.py:199-249).  Plain indexing: no kernel of ours."""
    if x.shape[0] != idx.shape[0]:
        raise ValueError("x and idx must have same batch dimension.")
    N, K = idx.shape[0], idx.shape[2]
    batch = torch.arange(N, device=x.device).view(N, 1, 1)
    x_out = x[batch, idx]                                              # [N, L, K, U]
    if lengths is not None:
        dead = torch.arange(K, device=x.device).view(1, 1, K) >= lengths.to(x.device).view(N, 1, 1)
        x_out = x_out.masked_fill(dead.unsqueeze(-1), 0.0)
    return x_out


def _check_cloud(points: torch.Tensor, lengths: Optional[torch.Tensor], normals: Optional[torch.Tensor]) -> torch.Tensor:
    """Shape checks of one side of the Chamfer inputs (chamfer_distance.py:33-57); returns the lengths (full clouds when None)."""
    if points.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    if lengths is None:
        lengths = torch.full((points.shape[0],), points.shape[1], dtype=torch.int64, device=points.device)
    elif lengths.ndim != 1 or lengths.shape[0] != points.shape[0]:
        raise ValueError("Expected lengths to be of shape (N,)")
    if normals is not None and normals.ndim != 3:
        raise ValueError("Expected normals to be of shape (N, P, 3")
    return lengths


class ChamferDistance(torch.nn.Module):
    """Per-point squared distances to the nearest neighbour in the other cloud, both directions (utils/chamfer_distance.py:60-159):
    returns (cham_x [N,P1], cham_y [N,P2], idx_x [N,P1], idx_y [N,P2]).  The reduction arguments are validated and, as in the
    reference, otherwise unused; normals are accepted and ignored (the reference never reads them either)."""

    def forward(self, x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, weights=None,
                batch_reduction: Union[str, None] = "mean", point_reduction: str = "mean"):
        if batch_reduction is not None and batch_reduction not in ["mean", "sum"]:
            raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
        if point_reduction not in ["mean", "sum"]:
            raise ValueError('point_reduction must be one of ["mean", "sum"]')
        x_lengths = _check_cloud(x, x_lengths, x_normals)
        y_lengths = _check_cloud(y, y_lengths, y_normals)
        N = x.shape[0]
        if y.shape[0] != N or y.shape[2] != x.shape[2]:
            raise ValueError("y does not have the correct shape.")
        if weights is not None:
            if weights.size(0) != N:
                raise ValueError("weights must be of shape (N,).")
            if bool((weights < 0).any()):
                raise ValueError("weights cannot be negative.")
            if float(weights.sum()) == 0.0:                      # all-zero weights: the reference returns zeros shaped by the reduction
                zero = (x.sum((1, 2)) * weights.view(N)) * 0.0
                return (zero.sum(), zero.sum()) if batch_reduction in ("mean", "sum") else (zero.view(N, 1), zero.view(N, 1))
        x_nn = knn_points(x, y, lengths1=x_lengths, lengths2=y_lengths, K=1)       # rows beyond a length are already zero
        y_nn = knn_points(y, x, lengths1=y_lengths, lengths2=x_lengths, K=1)
        cham_x = x_nn.dists[..., 0]
        cham_y = y_nn.dists[..., 0]
        if weights is not None:
            cham_x = cham_x * weights.view(N, 1)
            cham_y = cham_y * weights.view(N, 1)
        return cham_x, cham_y, x_nn.idx[..., -1], y_nn.idx[..., -1]


def chamfer_dist(tensor1: torch.Tensor, tensor2: torch.Tensor) -> torch.Tensor:
    """(sqrt(d(x->y)) + sqrt(d(y->x))) / 2 per point, clouds of equal size (utils/evaluation_depth.py:12-18)."""
    d1, d2, _, _ = ChamferDistance()(tensor1, tensor2)
    return (torch.sqrt(d1) + torch.sqrt(d2)) / 2


def _precision_recall(tensor1, tensor2, thresholds):
    d1, d2, _, _ = ChamferDistance()(tensor1, tensor2)
    precisions = torch.stack([(d1 < th).sum() / d1.numel() for th in thresholds]).to(tensor1.device)
    recalls = torch.stack([(d2 < th).sum() / d2.numel() for th in thresholds]).to(tensor1.device)
    return precisions, recalls


def auc(tensor1: torch.Tensor, tensor2: torch.Tensor, thresholds) -> torch.Tensor:
    """Area under the precision(recall) curve over the distance thresholds (utils/evaluation_depth.py:21-34).  As in the reference the
    thresholds are compared with SQUARED distances (what knn_points returns)."""
    precisions, recalls = _precision_recall(tensor1, tensor2, thresholds)
    return torch.trapz(precisions, recalls)


def f1_score(tensor1: torch.Tensor, tensor2: torch.Tensor, thresholds) -> torch.Tensor:
    """Mean over thresholds of F1 = 2 P R / (P + R) (0 where undefined), trapezoid rule (utils/evaluation_depth.py:74-91)."""
    precisions, recalls = _precision_recall(tensor1, tensor2, thresholds)
    f1 = 2 * precisions * recalls / (precisions + recalls)
    f1 = torch.where(torch.isnan(f1), torch.zeros_like(f1), f1)
    return torch.trapz(f1) / len(thresholds)


DICT_METRICS_3D = {                  # utils/evaluation_depth.py:109-125; gt / pred: [3, P] point sets of one image
    "MSE_3d": lambda gt, pred, thresholds: torch.norm(gt - pred, dim=0, p=2),
    "chamfer": lambda gt, pred, thresholds: chamfer_dist(gt.unsqueeze(0).permute(0, 2, 1), pred.unsqueeze(0).permute(0, 2, 1)),
    "F1": lambda gt, pred, thresholds: f1_score(gt.unsqueeze(0).permute(0, 2, 1), pred.unsqueeze(0).permute(0, 2, 1), thresholds=thresholds),
}


def eval_3d(gts: torch.Tensor, preds: torch.Tensor, masks: torch.Tensor, thresholds=None):
    """3-D metrics of a batch of point maps [B,3,H,W] under validity masks [B,1,H,W] (utils/evaluation_depth.py:160-182): maps are
    nearest-exact resampled so that about 240 x 320 valid points remain per batch, then per image MSE_3d, chamfer and F1 on the
    masked points.  The nearest-neighbour searches run in ud_knn_points."""
    import torch.nn.functional as F
    from collections import defaultdict
    summary = defaultdict(list)
    ratio = min(1.0, float((240 * 320 / masks.sum()) ** 0.5))
    h_max, w_max = int(gts.shape[-2] * ratio), int(gts.shape[-1] * ratio)
    gts = F.interpolate(gts, size=(h_max, w_max), mode="nearest-exact")
    preds = F.interpolate(preds, size=(h_max, w_max), mode="nearest-exact")
    masks = F.interpolate(masks.float(), size=(h_max, w_max), mode="nearest-exact").bool()
    for gt, pred, mask in zip(gts, preds, masks):
        if not torch.any(mask):
            continue
        for name, fn in DICT_METRICS_3D.items():
            summary[name].append(fn(gt[:, mask.squeeze()], pred[:, mask.squeeze()], thresholds).mean())
    return {name: torch.stack(vals, dim=0) for name, vals in summary.items()}


class RandomPatchExtractor(torch.nn.Module):
    """patch_size = (width, height) patches around `centers` [B,N,2] = (y, x), zero beyond the image border
    (modules/patch_extractor.py:16-42).  The result has the reference's shape {B, C, N, h, w} over memory written in [b][n][c][i][j]
    order (extract_patches_kernel.cu:22 vs :91) -- identical for the C = 1 tensors every reference call site passes."""

    def forward(self, tensor: torch.Tensor, centers: torch.Tensor, patch_size: Tuple[int, int]) -> torch.Tensor:
        if not tensor.is_cuda:
            raise RuntimeError("RandomPatchExtractor: GPU tensors expected (the HIP kernel is the only implementation)")
        dtype = tensor.dtype
        patch_width, patch_height = patch_size
        pad_w, pad_h = patch_width // 2, patch_height // 2
        B, Cc, H, W = tensor.shape
        N = centers.shape[1]
        # the reference shifts the centres into padded coordinates in the image dtype, then truncates (.int()) -- kept, so that
        # fractional / negative centres round the same way
        cpad = (centers.to(tensor.device) + torch.tensor([pad_h, pad_w], dtype=dtype, device=tensor.device).reshape(1, 1, 2)).int().contiguous()
        x = tensor.float().contiguous()
        out = torch.empty(B, Cc, N, patch_height, patch_width, device=tensor.device, dtype=torch.float32)
        d = mk(_lib.UdExtractPatches, in_=x, out=out, centers=cpad, B=B, C=Cc, H=H, W=W, N=N, h=patch_height, w=patch_width,
               pad_h=pad_h, pad_w=pad_w)
        check(_lib.lib.ud_extract_patches(d, cur_stream()), "ud_extract_patches")
        return out.to(dtype)


# ---- 2-D depth metrics (utils/evaluation_depth.py eval_depth, DICT_METRICS, DICT_METRICS_D) ----------------------------------------

EVAL_DEPTH_KEYS = ("d1_ssi", "d1_si", "d1", "d2", "d3", "rmse", "rmselog", "arel_ssi", "arel_si", "arel", "sqrel", "log10", "silog",
                   "medianlog", "d_auc", "tau_ssi", "tau_si", "tau")          # the reference's dict order = the rows of ud_eval_depth's out
_DAUC = {}


def _dauc_thresholds(device) -> torch.Tensor:
    """[1.25 ** e, e] for e = linspace(0.01, 5.0, 100) in fp32, made by torch on the device as the reference makes them; once per device."""
    key = (device.type, device.index)
    if key not in _DAUC:
        e = torch.linspace(0.01, 5.0, steps=100, device=device)
        _DAUC[key] = torch.cat([1.25 ** e, e]).contiguous()
    return _DAUC[key]


def _eval_depth_rows(gt: torch.Tensor, pred: torch.Tensor, mask: Optional[torch.Tensor], max_depth) -> torch.Tensor:
    """ud_eval_depth on fp32 gt [B,H,W], pred [B,h,w], u8 mask [B,H,W] or None -> fp32 [18, B] (rows in EVAL_DEPTH_KEYS order)."""
    B, H, W = gt.shape
    h, w = pred.shape[1:]
    dev = gt.device
    nbytes = int(_lib.lib.ud_eval_depth_work_bytes(B, H, W))
    if nbytes < 0:
        raise ValueError(f"eval_depth: unsupported sizes B={B} H={H} W={W}")
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    out = torch.empty(len(EVAL_DEPTH_KEYS), B, device=dev, dtype=torch.float32)
    d = mk(_lib.UdEvalDepth, gt=gt, pred=pred, mask=mask, thresholds=_dauc_thresholds(dev), out=out, work=work, B=B, H=H, W=W, h=h, w=w,
           max_depth=0.0 if max_depth is None else float(max_depth), has_max_depth=0 if max_depth is None else 1, work_bytes=nbytes)
    check(_lib.lib.ud_eval_depth(d, cur_stream()), "ud_eval_depth")
    return out


def eval_depth(gts: torch.Tensor, preds: torch.Tensor, masks: torch.Tensor, max_depth=None):
    """Per-image depth metrics of a batch (utils/evaluation_depth.py:132-147): gts [B,1,H,W], preds [B,1,h,w] (bilinearly resampled to
    H x W, align_corners=False), masks [B,1,H,W] bool; valid pixels = mask & (gt <= max_depth when given).  Returns the reference's 18
    keys in its order, each a [B] fp32 GPU tensor: d1..d3, rmse, rmselog, arel, sqrel, log10, silog, medianlog, d_auc, tau on the
    prediction, and d1 / arel / tau again after the least-squares scale-and-shift (_ssi) and the median scale (_si) alignment.  An
    image without a valid pixel gives NaN everywhere, as in the reference.  One ud_eval_depth call: no host synchronisation, bitwise
    reproducible.  Inputs of another float dtype are converted to fp32 first (the reference computes in the input dtype)."""
    for name, t in (("gts", gts), ("preds", preds), ("masks", masks)):
        if not isinstance(t, torch.Tensor) or t.ndim != 4 or t.shape[1] != 1:
            raise ValueError(f"eval_depth: {name} must be [B,1,H,W], got {tuple(getattr(t, 'shape', ()))}")
    B = gts.shape[0]
    if B == 0:
        raise ValueError("eval_depth: empty batch")
    if preds.shape[0] != B or masks.shape[0] != B:
        raise ValueError(f"eval_depth: batch sizes differ (gts {B}, preds {preds.shape[0]}, masks {masks.shape[0]})")
    if masks.shape != gts.shape:
        raise ValueError(f"eval_depth: masks {tuple(masks.shape)} must match gts {tuple(gts.shape)}")
    H, W = gts.shape[-2:]
    if H * W > 0 and preds.shape[-2] * preds.shape[-1] == 0:
        raise ValueError("eval_depth: empty prediction")
    if not (gts.is_cuda and preds.is_cuda and masks.is_cuda):
        raise RuntimeError("eval_depth: GPU tensors expected (the HIP kernels are the only implementation)")
    gt = gts.reshape(B, H, W).float().contiguous()
    pred = preds.reshape(B, preds.shape[-2], preds.shape[-1]).float().contiguous()
    mask = masks.reshape(B, H, W).to(torch.bool).contiguous().view(torch.uint8)
    out = _eval_depth_rows(gt, pred, mask, max_depth)
    return {name: out[k] for k, name in enumerate(EVAL_DEPTH_KEYS)}


def _metric_1d(name: str):
    row = EVAL_DEPTH_KEYS.index(name)

    def fn(gt: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
        if gt.ndim != 1 or pred.shape != gt.shape:
            raise ValueError(f"DICT_METRICS[{name!r}]: 1-D gt and pred of equal length expected")
        if not (gt.is_cuda and pred.is_cuda):
            raise RuntimeError(f"DICT_METRICS[{name!r}]: GPU tensors expected (the HIP kernels are the only implementation)")
        n = gt.shape[0]
        out = _eval_depth_rows(gt.float().contiguous().view(1, 1, n), pred.float().contiguous().view(1, 1, n), None, None)
        return out[row, 0]

    fn.__name__ = name
    return fn


# utils/evaluation_depth.py:93-110: metric(gt, pred) on the 1-D valid pixels of one image -> 0-d tensor; each is one image of 1 x n
# through ud_eval_depth (no mask, no resample)
DICT_METRICS = {name: _metric_1d(name) for name in ("d1", "d2", "d3", "rmse", "rmselog", "arel", "sqrel", "log10", "silog", "medianlog",
                                                    "d_auc", "tau")}

DICT_METRICS_D = {           # utils/evaluation_depth.py:124-129: per-pixel maps (plain torch, not on a hot path)
    "a1": lambda gt, pred: (torch.maximum((gt / pred), (pred / gt)) > 1.25 ** 1.0).to(torch.float32),
    "abs_rel": lambda gt, pred: (torch.abs(gt - pred) / gt),
}


# ---- 3-D metrics of a batch on the device (utils/evaluation_depth.py eval_3d; datasets/base_dataset.py accumulate_metrics_3d) -----------

EVAL_3D_KEYS = ("MSE_3d", "chamfer", "F1")                                # the reference's dict order = the rows of ud_eval_3d's out


def eval_3d_size(H: int, W: int, n_valid: int) -> Tuple[int, int]:
    """The size (h, w) eval_3d resamples [.., H, W] maps to when the batch has n_valid valid pixels, in the reference's arithmetic:
    ratio = min(1.0, (240 * 320 / masks.sum()) ** 0.5) is an fp32 tensor there, so the quotient, the square root and the products
    H * ratio, W * ratio are fp32 and int() truncates them.  Pure host code (numpy float32); ud_eval_3d computes the same on the
    device.  n_valid = 0 gives (H, W): every image is empty anyway."""
    if n_valid <= 0:
        return int(H), int(W)
    q = np.float32(76800.0) / np.float32(n_valid)
    r = np.float32(np.sqrt(np.float64(q)))             # through fp64 and back: the correctly rounded fp32 square root
    if r >= np.float32(1.0):
        return int(H), int(W)
    return int(np.float32(H) * r), int(np.float32(W) * r)


def thresholds_3d(min_depth: float, max_depth: float, device=None) -> torch.Tensor:
    """The 100 F1 thresholds of accumulate_metrics_3d (datasets/base_dataset.py): linspace(log(min_depth), log(max_depth / 20), 100).exp(),
    fp32, made by torch on `device` as the reference makes them."""
    return torch.linspace(math.log(min_depth), math.log(max_depth / 20), 100, device=device).exp()


def eval_3d_batch(gts: torch.Tensor, preds: torch.Tensor, masks: torch.Tensor, thresholds):
    """eval_3d (utils/evaluation_depth.py:160-182) for a whole batch in one ud_eval_3d call: gts, preds [B,3,H,W], masks [B,1,H,W] or
    [B,H,W] (bool, or any dtype with nonzero = valid), thresholds a list of floats or a tensor [T] (converted to fp32 once, compared
    with SQUARED distances as in the reference, any order).  Returns {"MSE_3d", "chamfer", "F1"}, each fp32 [B], plus "count" int64 [B]
    (the points of every image after the resample) and "size" int32 [2] (the resample size (h, w) = eval_3d_size(H, W, masks.sum())).
    Every tensor stays on the GPU and nothing synchronises: the valid count, the size, the nearest-exact resample, the compaction, the
    two nearest-neighbour searches per image (each direction once) and the metrics are eight stream-ordered launches.  Bitwise
    reproducible.

    An image without a valid sample has count 0 and NaN in the three rows.  The reference's eval_3d skips such images and so returns
    fewer rows: out[name][out["count"] > 0] is what it returns.  The size follows the reference's fp32 rule; eval_ops.eval_3d above
    multiplies in fp64 and is one pixel smaller for some sizes (518 x 518 x 3 fully valid: 159 instead of 160).  Inputs of another
    float dtype are converted to fp32 and non-contiguous views are made contiguous first."""
    for name, t in (("gts", gts), ("preds", preds)):
        if not isinstance(t, torch.Tensor) or t.ndim != 4 or t.shape[1] != 3:
            raise ValueError(f"eval_3d_batch: {name} must be [B,3,H,W], got {tuple(getattr(t, 'shape', ()))}")
        if not t.is_floating_point():
            raise ValueError(f"eval_3d_batch: {name} must be a float tensor, got {t.dtype}")
    if preds.shape != gts.shape:
        raise ValueError(f"eval_3d_batch: preds {tuple(preds.shape)} must match gts {tuple(gts.shape)}")
    B, _, H, W = gts.shape
    if B == 0 or H * W == 0:
        raise ValueError("eval_3d_batch: empty batch or empty maps")
    if not isinstance(masks, torch.Tensor) or tuple(masks.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"eval_3d_batch: masks must be [B,1,H,W] or [B,H,W] matching gts, got {tuple(getattr(masks, 'shape', ()))}")
    if isinstance(thresholds, torch.Tensor):
        if thresholds.ndim != 1 or thresholds.is_complex():
            raise ValueError(f"eval_3d_batch: thresholds must be a 1-D real tensor, got {tuple(thresholds.shape)} {thresholds.dtype}")
        T = thresholds.shape[0]
    else:
        try:
            thresholds = [float(v) for v in thresholds]
        except TypeError as e:
            raise ValueError("eval_3d_batch: thresholds must be a list of floats or a 1-D tensor") from e
        T = len(thresholds)
    if not 1 <= T <= _lib.UD_EVAL3D_MAX_T:
        raise ValueError(f"eval_3d_batch: 1 <= len(thresholds) <= {_lib.UD_EVAL3D_MAX_T} expected, got {T}")
    if B > _lib.UD_EVAL3D_MAX_B:
        raise ValueError(f"eval_3d_batch: at most {_lib.UD_EVAL3D_MAX_B} images per call, got {B}")
    nbytes = int(_lib.lib.ud_eval_3d_work_bytes(B, H, W, T))
    if nbytes < 0:
        raise ValueError(f"eval_3d_batch: unsupported sizes B={B} H={H} W={W} T={T}")
    if not (gts.is_cuda and preds.is_cuda and masks.is_cuda):
        raise RuntimeError("eval_3d_batch: GPU tensors expected (the HIP kernels are the only implementation)")
    dev = gts.device
    th = torch.as_tensor(thresholds, device=dev).to(torch.float32).contiguous()
    gt = gts.float().contiguous()
    pred = preds.float().contiguous()
    mask = masks.reshape(B, H, W).to(torch.bool).contiguous().view(torch.uint8)
    out = torch.empty(len(EVAL_3D_KEYS), B, device=dev, dtype=torch.float32)
    counts = torch.empty(B, device=dev, dtype=torch.int64)
    size = torch.empty(2, device=dev, dtype=torch.int32)
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    d = mk(_lib.UdEval3d, gt=gt, pred=pred, mask=mask, thresholds=th, out=out, counts=counts, size=size, work=work, work_bytes=nbytes,
           B=B, H=H, W=W, T=T)
    check(_lib.lib.ud_eval_3d(d, cur_stream()), "ud_eval_3d")
    res = {name: out[k] for k, name in enumerate(EVAL_3D_KEYS)}
    res["count"] = counts
    res["size"] = size
    return res


class MetricsAccumulator:
    """The reference's metrics_store / metrics_count / get_evaluation (datasets/base_dataset.py:219-271) for ONE process: the rows of
    every batch are kept on the device and reduced once at the end of the dataset.

        acc = MetricsAccumulator(min_depth, max_depth)
        for batch in loader:
            acc.accumulate_depth(gts, preds, masks)            # eval_depth's 18 rows, masked at max_depth
            acc.accumulate_3d(gt_points, pred_points, masks)   # eval_3d_batch's 3 rows with thresholds_3d(min_depth, max_depth)
            # or both, with the ground-truth points made from the depth and the camera:  acc.accumulate_metrics(inputs, preds)
        metrics = acc.get_evaluation()                         # {key: round(mean, 5)}; the only place that synchronises

    3-D keys average over the rows with count > 0, because the reference never stored the others; depth keys average plainly, as the
    reference does, so a NaN row (an image without a valid pixel) propagates.  The cross-rank gather of the reference
    (sync_tensor_across_gpus before the mean) is out of scope: every process reduces what it accumulated."""

    def __init__(self, min_depth: float = 0.01, max_depth: float = 1000.0):
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self._rows = {}                                  # key -> list of [B] tensors
        self._keep = {}                                  # key -> list of [B] bool tensors (3-D keys only)
        self._thresholds = {}

    def accumulate_depth(self, gts: torch.Tensor, preds: torch.Tensor, masks: torch.Tensor, name: str = "") -> None:
        for key, row in eval_depth(gts, preds, masks, max_depth=self.max_depth).items():
            self._rows.setdefault(f"{name}_{key}".strip("_"), []).append(row)

    def accumulate_3d(self, gts: torch.Tensor, preds: torch.Tensor, masks: torch.Tensor, name: str = "") -> None:
        dev = (gts.device.type, gts.device.index)
        if dev not in self._thresholds:
            self._thresholds[dev] = thresholds_3d(self.min_depth, self.max_depth, device=gts.device)
        res = eval_3d_batch(gts, preds, masks, self._thresholds[dev])
        keep = res["count"] > 0
        for key in EVAL_3D_KEYS:
            full = f"{name}_{key}".strip("_")
            self._rows.setdefault(full, []).append(res[key])
            self._keep.setdefault(full, []).append(keep)

    def accumulate_metrics(self, inputs: dict, preds: dict, keyframe_idx: Optional[int] = None) -> None:
        """The reference's accumulate_metrics (datasets/base_dataset.py:186-216) for depth and points: inputs holds "depth",
        "depth_mask", "camera" (and "camera_original" when the ground truth is at the raw image's size; optionally "points",
        "points_mask"), preds the prediction tensors by key.  Ground-truth points are added first when inputs has a depth and no points
        (gtpoints.add_points); with keyframe_idx only that image of the batch is evaluated; every prediction key that contains "depth"
        goes through accumulate_depth, every key that contains "points" through accumulate_3d (points_mask if present, else
        depth_mask), each under the name the reference derives from the key.  A metric missing from either side is skipped."""
        if "depth" in inputs and "points" not in inputs:
            from .gtpoints import add_points
            inputs = add_points(inputs)
        available = [m for m in ("depth", "points") if any(m in k for k in inputs) and any(m in k for k in preds)]
        sl = slice(None) if keyframe_idx is None else slice(keyframe_idx, keyframe_idx + 1)
        if "depth" in available:
            gts, masks = inputs["depth"][sl], inputs["depth_mask"][sl].bool()
            for key, pred in preds.items():
                if "depth" in key:
                    self.accumulate_depth(gts, pred[sl], masks, name=key.replace("depth", "").strip("-").strip("_"))
        if "points" in available:
            gts, masks = inputs["points"][sl], inputs.get("points_mask", inputs["depth_mask"])[sl].bool()
            for key, pred in preds.items():
                if "points" in key:
                    self.accumulate_3d(gts, pred[sl], masks, name=key.replace("points", "").strip("-").strip("_"))

    def get_evaluation(self) -> dict:
        """{key: round(mean over the accumulated rows, 5)}; clears the store."""
        out = {}
        for key, rows in self._rows.items():
            v = torch.cat(rows)
            if key in self._keep:
                v = v[torch.cat(self._keep[key])]
            out[key] = float(np.round(v.mean().item(), 5))
        self._rows, self._keep = {}, {}
        return out
