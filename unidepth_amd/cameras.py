"""Ground-truth camera models accepted by UniDepthV2.infer(rgb, camera=...) besides a [...,3,3] pinhole K tensor
(SURVEY.md 8f next-3).  Parameter conventions follow the reference classes of the same names (unidepth/utils/camera.py):

    Pinhole(K)                                   # utils/camera.py:229-266
    EUCM(params=[fx, fy, cx, cy, alpha, beta])   # enhanced unified camera model, utils/camera.py:276-328
    Spherical(params=[fx, fy, cx, cy, W, H, hfov/2, vfov/2])   # equirectangular panorama (angles in rad), :331-410
    OPENCV(params=[fx, fy, cx, cy, k1..k6, p1, p2, s1..s4])    # radial (k1..k3; k4..k6 must be 0) + tangential + thin prism, :412-694
    Fisheye624(params=[fx, fy, cx, cy, k1..k6, p1, p2, s1..s4])  # 6-coefficient fisheye + tangential + thin prism, :697-974
    MEI(params=[fx, fy, cx, cy, k1, k2, p1, p2, xi])           # unified omnidirectional model, :977-1082

Only what the infer() path needs is here: the bookkeeping that maps a camera of the ORIGINAL image to the network input
(aspect padding = a crop by negative offsets, then the resize factor; utils/camera.py:78-81,115-120 and the Spherical overrides
:336-357) and a tag for the ray kernel (ud_rays_from_kinv gt_mode).  The unprojection itself runs on the GPU
(csrc/pointwise.hip rays_kernel; the iterative models -- OPENCV, Fisheye624, MEI -- through ud_rays_from_camera, which
reproduces the reference's Newton / trust-region solvers including the image-wide early exit of the radial loop).  Unlike the reference, infer() does not modify the camera object it is given.
Camera.reconstruct(depth), on every class, is the ground-truth point map of the validation loop (gtpoints.py, csrc/reconstruct.hip).
Camera.project(points) / get_projection_mask(), on every class, go the other way (reproject.project_camera, csrc/project.hip).
Camera.unproject(uv) / get_rays(shapes), on every class, are the rays at arbitrary image coordinates and of the pixel grid
(unproject.unproject_camera, csrc/unproject.hip); unproject remembers the reference's unprojection_mask.
Camera.get_overlap_mask() is the reference's mask_overlap_projection of the last project() call, for the two classes whose project sets
it there, OPENCV and Fisheye624 (remap.overlap_mask, csrc/remap.hip).
Objects of the reference's own classes are accepted as well (matched by class name and `.params`)."""
from __future__ import annotations

import torch

GT_PINHOLE, GT_EUCM, GT_SPHERICAL, GT_OPENCV, GT_FISHEYE624, GT_MEI = 1, 2, 3, 4, 5, 6


class Camera:
    gt_mode = 0
    n_params = 4
    projection_mask = None                            # the mask of the last project() call (get_projection_mask)
    unprojection_mask = None                          # the mask of the last unproject() call, where the class sets one
    overlap_mask = None                               # mask_overlap_projection of the last project() call, where the class sets one

    def __init__(self, params: torch.Tensor):
        params = torch.as_tensor(params, dtype=torch.float32)
        if params.ndim == 1:
            params = params.unsqueeze(0)
        assert params.shape[-1] == self.n_params, f"{type(self).__name__} takes {self.n_params} parameters"
        self.params = params.clone()

    @property
    def K(self) -> torch.Tensor:
        K = torch.eye(3).repeat(self.params.shape[0], 1, 1)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = self.params[:, 0], self.params[:, 1], self.params[:, 2], self.params[:, 3]
        return K

    def network_params(self, paddings, resize_factor: float) -> torch.Tensor:
        """Parameters after `crop(-pad)` and `resize(rf)` (reference unidepthv2.py:299-303), [n, n_params] fp32."""
        pl, pr, pt, pb = paddings
        p = self.params.clone()
        p[:, 2] += pl
        p[:, 3] += pt
        p[:, :4] *= resize_factor
        return p

    def reconstruct(self, depth: torch.Tensor) -> torch.Tensor:
        """The reference's Camera.reconstruct: depth [B,1,H,W] or [B,H,W] on the GPU -> ground-truth points fp32 [B,3,H,W]
        (gtpoints.gt_points, csrc/reconstruct.hip).  The camera is not modified."""
        from .gtpoints import gt_points
        return gt_points(depth, self)

    def project(self, points: torch.Tensor) -> torch.Tensor:
        """The reference's Camera.project: points fp32 [B,3,H,W] on the GPU -> image coordinates fp32 [B,2,H,W], every image through its
        own camera in one launch (reproject.project_camera, csrc/project.hip).  The image the mask is taken against is the point map's
        own (H, W), as in the reference.  Remembers the mask of this call for get_projection_mask() and, for OPENCV and Fisheye624 (the
        classes whose project sets it in the reference), the overlap mask of uv for get_overlap_mask(); nothing else of the camera changes."""
        from .reproject import project_camera
        if not isinstance(points, torch.Tensor) or points.ndim != 4 or points.shape[1] != 3:
            raise ValueError(f"{type(self).__name__}.project: points must be [B,3,H,W], got {tuple(getattr(points, 'shape', ()))}")
        if not points.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.project: GPU tensors expected (the HIP kernels are the only implementation)")
        uv, inside, _ = project_camera(points, self)
        self.projection_mask = self._projection_mask(inside.unsqueeze(1))
        self.overlap_mask = self._overlap_mask(uv)
        return uv

    def _projection_mask(self, inside: torch.Tensor):
        return inside

    def _overlap_mask(self, uv: torch.Tensor):
        return None

    def unproject(self, uv: torch.Tensor) -> torch.Tensor:
        """The reference's Camera.unproject: image coordinates [B,2,H,W] (or [B,N,2]) on the GPU -> the class's own rays fp32 [B,3,H,W]
        ([B,N,3]), not normalised, every image through its own camera (unproject.unproject_camera, csrc/unproject.hip).  A batch-1 uv
        goes through every camera, as the reference's BatchCamera concatenates its members' results.  Sets self.unprojection_mask: bool
        [B,1,H,W] ([B,N]) for Pinhole (z > 1e-4) and EUCM (the model's domain; the reference's lacks the channel axis), None for the
        classes that set none; for a BatchCamera every image follows its member's rule (True for the members without one)."""
        from .unproject import unproject_camera
        if not isinstance(uv, torch.Tensor):
            raise ValueError(f"{type(self).__name__}.unproject: uv must be a tensor")
        rays, mask = unproject_camera(uv, self, return_mask=True)
        self.unprojection_mask = self._unprojection_mask(mask)
        return rays

    def _unprojection_mask(self, mask: torch.Tensor):
        return None

    def get_rays(self, shapes) -> torch.Tensor:
        """The reference's Camera.get_rays: shapes = (B, H, W) or (H, W) -> the normalised rays fp32 [B,3,H,W] of the pixel centres."""
        from .unproject import get_rays
        return get_rays(self, shapes)

    def get_projection_mask(self):
        """The mask of the last project() call, bool [B,1,H,W], with the reference's returns class by class:

            EUCM, OPENCV, Fisheye624, MEI   True where the point projects into the image (EUCM: and z >= 0)
            Pinhole                         INVERTED, deliberately: the reference names its inside test `invalid` and stores `~invalid`
                                            (utils/camera.py:245-251), so True marks the points that fall OUTSIDE the image
            Spherical                       None: the reference's project sets no mask
            BatchCamera                     every image with its member's rule; a Spherical member gets the plain inside test (the
                                            reference would fail there, on torch.cat of None)

        None before the first project()."""
        return self.projection_mask

    def get_overlap_mask(self):
        """The reference's mask_overlap_projection of the last project() call, bool [B,1,H,W] (remap.overlap_mask): False where the
        projection folds content from another part of the image over the pixel.  OPENCV and Fisheye624 set it, as in the reference (MEI's
        call is commented out there); None for Pinhole, EUCM, Spherical and MEI, and before the first project().  BatchCamera: with at
        least one OPENCV / Fisheye624 member every image follows its member's rule (all True for the members without one), else None."""
        return self.overlap_mask


class Pinhole(Camera):
    gt_mode = GT_PINHOLE

    def __init__(self, K: torch.Tensor = None, params: torch.Tensor = None):
        if params is None:
            K = torch.as_tensor(K, dtype=torch.float32).reshape(-1, 3, 3)
            params = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], dim=1)
        super().__init__(params)

    def _projection_mask(self, inside):
        return ~inside                                # the reference's inversion, see get_projection_mask

    def _unprojection_mask(self, mask):
        return mask


class EUCM(Camera):
    gt_mode = GT_EUCM
    n_params = 6

    def _unprojection_mask(self, mask):
        return mask


class Spherical(Camera):
    gt_mode = GT_SPHERICAL
    n_params = 8

    def _projection_mask(self, inside):
        return None

    def network_params(self, paddings, resize_factor: float) -> torch.Tensor:
        pl, pr, pt, pb = paddings
        p = self.params.clone()
        W, H = p[:, 4].clone(), p[:, 5].clone()
        p[:, 2] += pl
        p[:, 3] += pt
        p[:, 4] = W + pl + pr                    # a padded panorama spans proportionally more angle
        p[:, 5] = H + pt + pb
        p[:, 6] *= (W + pl + pr) / W
        p[:, 7] *= (H + pt + pb) / H
        p[:, :6] *= resize_factor
        return p


class _SingleCamera(Camera):
    """The iterative models unproject one camera at a time in the reference (`B` is taken from the pixel grid, which has batch
    1: utils/camera.py:498-509), so one parameter row is what infer() can be given."""

    def __init__(self, params: torch.Tensor):
        super().__init__(params)
        assert self.params.shape[0] == 1, f"{type(self).__name__}: one camera per infer() call (as in the reference)"


class OPENCV(_SingleCamera):
    gt_mode = GT_OPENCV
    n_params = 16

    def __init__(self, params: torch.Tensor):
        super().__init__(params)
        assert float(self.params[..., 7:10].abs().sum()) == 0.0, "Do not support poly division model"   # utils/camera.py:416-418

    def _overlap_mask(self, uv):
        from .remap import overlap_mask
        return overlap_mask(uv)


class Fisheye624(_SingleCamera):
    gt_mode = GT_FISHEYE624
    n_params = 16

    def _overlap_mask(self, uv):
        from .remap import overlap_mask
        return overlap_mask(uv)


class MEI(_SingleCamera):
    gt_mode = GT_MEI
    n_params = 9


class BatchCamera(Camera):
    """Several cameras, one per image of the batch, possibly of DIFFERENT models (the reference's wrapper utils/camera.py:1145-1308: its
    unproject() concatenates every member's own unproject, :1166-1171; infer() crops / resizes each member, :1173-1186).  Members are
    single-camera objects of the classes above.  uniform(): the same cameras as ONE batched object when every member is of one closed-form
    class (Pinhole / EUCM / Spherical), which the batched ray kernel takes; None otherwise (the plan then records one ray launch per image)."""
    gt_mode = -1

    def __init__(self, cameras):
        self.cameras = list(cameras)
        assert self.cameras and all(isinstance(c, Camera) and not isinstance(c, BatchCamera) and c.params.shape[0] == 1 for c in self.cameras), \
            "BatchCamera: a non-empty list of single cameras"
        self.params = torch.zeros(len(self.cameras), 16)
        for i, c in enumerate(self.cameras):
            self.params[i, : c.params.shape[1]] = c.params[0]

    @property
    def gt_modes(self):
        return tuple(c.gt_mode for c in self.cameras)

    def _projection_mask(self, inside):
        flip = torch.tensor([isinstance(c, Pinhole) for c in self.cameras]).to(inside.device)
        return inside ^ flip[:, None, None, None]

    def _unprojection_mask(self, mask):
        return mask

    def _overlap_mask(self, uv):
        sets = [isinstance(c, (OPENCV, Fisheye624)) for c in self.cameras]
        if not any(sets):
            return None
        from .remap import overlap_mask
        return overlap_mask(uv) | ~torch.tensor(sets).to(uv.device)[:, None, None, None]

    def uniform(self):
        cls = type(self.cameras[0])
        if cls in (Pinhole, EUCM, Spherical) and all(type(c) is cls for c in self.cameras):
            p = torch.cat([c.params for c in self.cameras], dim=0)
            return Pinhole(params=p) if cls is Pinhole else cls(p)
        return None


def _flatten(cams):
    out = []
    for c in cams:
        out.extend(_flatten(c) if isinstance(c, (list, tuple)) else [c])
    return out


_BY_NAME = {"Pinhole": Pinhole, "EUCM": EUCM, "Spherical": Spherical, "OPENCV": OPENCV, "Fisheye624": Fisheye624, "MEI": MEI}


def as_camera(obj) -> Camera:
    """Own classes pass through; reference-class instances (or anything with a matching class name and `.params`) are wrapped."""
    if isinstance(obj, Camera):
        return obj
    name = type(obj).__name__
    if name == "BatchCamera" and getattr(obj, "cameras", None):
        cams = [as_camera(c) for c in _flatten(obj.cameras)]
        return cams[0] if len(cams) == 1 else BatchCamera(cams)
    cls = _BY_NAME.get(name)
    if cls is None or not hasattr(obj, "params"):
        raise NotImplementedError(f"camera model '{name}' is not implemented ({', '.join(_BY_NAME)} are)")
    if cls is Pinhole:
        return Pinhole(params=torch.as_tensor(obj.params, dtype=torch.float32)[..., :4])
    return cls(torch.as_tensor(obj.params, dtype=torch.float32))
