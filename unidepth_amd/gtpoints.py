"""Ground-truth point maps for the validation loop: the reference's Camera.reconstruct (unidepth/utils/camera.py) and
base_dataset.add_points (datasets/base_dataset.py:180-184) for a whole batch in one ud_reconstruct call (csrc/reconstruct.hip).

    gt_points(depth, camera)      fp32 [B,3,H,W] from a ground-truth depth and a ground-truth camera, one camera model per image
    prepare_camera(camera, B, device)   the camera's parameter rows uploaded once (needed under graph capture, useful in a loop)
    add_points(inputs)            inputs["points"] from inputs.get("camera_original", inputs["camera"]) and inputs["depth"]

eval_ops.MetricsAccumulator.accumulate_metrics runs the reference's whole accumulate_metrics on top of these.  The HIP kernels are
the only implementation: CPU tensors raise.

The camera must describe the image the depth map belongs to.  prepare_test_batch returns the camera of the network-sized image;
when the ground truth is kept at the raw image's size the caller supplies that camera as inputs["camera_original"], as the
reference's datasets do."""
from __future__ import annotations

import torch

from . import _args, _lib
from ._args import PreparedCamera
from .cameras import BatchCamera, GT_PINHOLE, as_camera
from .ops import check, cur_stream, mk


def _pinhole_rows(K: torch.Tensor, B: int) -> torch.Tensor:
    if K.ndim == 2:
        K = K[None]
    if K.ndim != 3 or tuple(K.shape[-2:]) != (3, 3) or not K.is_floating_point():
        raise ValueError(f"gt_points: an intrinsics tensor must be a float [3,3] or [B,3,3], got {tuple(K.shape)} {K.dtype}")
    _args.batch_of("gt_points", "camera", K.shape[0], B)
    K = K.to(torch.float32)
    rows = torch.zeros(K.shape[0], 16, dtype=torch.float32, device=K.device)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    # the closed-form inverse has no skew term.  A host tensor is checked here; a device tensor cannot be read without a
    # synchronisation, so a skewed matrix there turns its image's row into NaN and every point of that image comes back NaN
    if not K.is_cuda:
        if bool((K[:, 0, 1] != 0).any()):
            raise ValueError("gt_points: intrinsics with a non-zero skew K[0,1] are not supported (the closed-form inverse has no skew term)")
    else:
        rows = torch.where((K[:, 0, 1] != 0)[:, None], torch.full_like(rows, float("nan")), rows)
    return rows


def prepare_camera(camera, B: int, device) -> PreparedCamera:
    """The parameter rows of `camera` for a batch of B images, on `device`.  camera: a [3,3] / [B,3,3] intrinsics tensor (zero skew: ValueError on the host, NaN points on the device),
    a Pinhole / EUCM / Spherical with 1 or B rows, one OPENCV / Fisheye624 / MEI (applied to every image), a BatchCamera of B
    members of any mix of models, or objects of the reference's classes (cameras.as_camera).  The camera is not modified."""
    if isinstance(camera, PreparedCamera):
        _args.batch_of("gt_points", "camera", len(camera), B, shared=False)
        return camera
    if isinstance(camera, torch.Tensor):
        rows, models = _pinhole_rows(camera, B), (GT_PINHOLE,)
    else:
        cam = as_camera(camera)
        if isinstance(cam, BatchCamera):
            rows, models = cam.params, cam.gt_modes
            _args.batch_of("gt_points", "camera", len(models), B, shared=False)
        else:
            n, k = cam.params.shape
            _args.batch_of("gt_points", "camera", n, B)
            rows = torch.zeros(n, 16, dtype=torch.float32, device=cam.params.device)
            rows[:, :k] = cam.params
            models = (cam.gt_mode,)
    _args.max_images("gt_points", B)
    _args.one_gpu("gt_points", torch.device(device))
    rows = rows.to(device=device, dtype=torch.float32)
    if rows.shape[0] != B:
        rows = rows.expand(B, 16)
    return PreparedCamera(rows.contiguous(), models if len(models) == B else models * B)


def gt_points(depth: torch.Tensor, camera) -> torch.Tensor:
    """Camera.reconstruct for a batch: depth [B,1,H,W] or [B,H,W] (any float dtype, any layout; converted to contiguous fp32 first)
    and a camera as prepare_camera takes it -> points fp32 [B,3,H,W].  Per model (pixel centres u + 0.5, v + 0.5):

        Pinhole              K^-1 [u, v, 1] * max(depth, 0)
        Spherical            the unit-sphere direction * depth (a negative depth passes through)
        EUCM, OPENCV, Fisheye624, MEI    r / max(r.z, 1e-4) * max(depth, 1e-4), r the model's unproject (not normalised)

    A NaN depth or parameter gives NaN.  One launch for a batch of closed-form models and MEI; with OPENCV / Fisheye624 members at
    most 12, whatever B is, each such image leaving the radial loop on its own as the members of the reference's BatchCamera do.
    Stream-ordered, nothing synchronises.  Camera objects and host tensors are uploaded with one small copy, which a graph capture
    does not allow: capture with a prepare_camera() result or with an intrinsics tensor that is already on the device.  A skewed
    intrinsics tensor raises ValueError when it is on the host; on the device its images come back NaN (no read-back)."""
    B, H, W = _args.depth_map("gt_points", "depth", depth)
    _args.max_images("gt_points", B)
    if _lib.lib.ud_reconstruct_work_bytes(B, H, W, 0) < 0:
        raise ValueError(f"gt_points: unsupported sizes B={B} H={H} W={W}")
    cam = prepare_camera(camera, B, depth.device)
    _args.one_gpu("gt_points", depth.device, cam.params)
    d = depth.reshape(B, 1, H, W).float().contiguous()
    points = torch.empty(B, 3, H, W, device=d.device, dtype=torch.float32)
    n_iter = _args.n_iterative(cam)
    nbytes = int(_lib.lib.ud_reconstruct_work_bytes(B, H, W, n_iter))
    work = torch.empty(nbytes, device=d.device, dtype=torch.uint8) if nbytes else None
    desc = mk(_lib.UdReconstruct, depth=d, params=cam.params, points=points, work=work, work_bytes=nbytes, B=B, H=H, W=W)
    _args.set_models(desc.model, cam)
    with torch.cuda.device(d.device):
        check(_lib.lib.ud_reconstruct(desc, cur_stream()), "ud_reconstruct")
    return points


def add_points(inputs: dict) -> dict:
    """base_dataset.add_points: inputs["points"] = camera.reconstruct(inputs["depth"]) with inputs["camera_original"] when present
    (the ground truth at the raw image's size), else inputs["camera"].  Returns inputs."""
    inputs["points"] = gt_points(inputs["depth"], inputs.get("camera_original", inputs["camera"]))
    return inputs
