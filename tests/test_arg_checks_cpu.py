"""The argument checks of the camera-map wrappers (unidepth_amd/_args.py), one table for the whole family, no GPU: every check below
fires before the device check, so CPU tensors reach it.  Per case: the exception is a ValueError, its message starts with the public
name of the function called, it names the offending argument, and -- with the argument's name, shapes, dtypes and numbers blanked --
it is the one sentence the family uses for that kind of fault, whichever function reports it.

Not in the table, because a CPU call cannot reach them: the transform of project_camera and render_depth_camera and their image count
(both functions need the camera's rows on the device before they look at either)."""
import re

import pytest
import torch

from unidepth_amd import _lib, cameras, consistency, gtpoints, normals, remap, reproject, unproject, warp

K = torch.tensor([[50.0, 0, 2.0], [0, 51.0, 1.5], [0, 0, 1]])
B, H, W = 2, 3, 4
MANY = _lib.UD_RECON_MAX_B + 1
depth, points, rows = torch.rand(B, 1, H, W) + 1, torch.rand(B, 3, H, W), torch.rand(B, 5, 3)
uv, uv3, src = torch.rand(B, 2, H, W), torch.rand(3, 2, H, W), torch.rand(B, 3, H, W)
views, cams, T = torch.rand(B, 2, H, W) + 1, [K, K], torch.eye(4).repeat(2, 1, 1)
ints, floats, bools = torch.ones(B, 1, H, W, dtype=torch.int32), torch.ones(B, 1, H, W), torch.ones(B, 1, H, W, dtype=torch.bool)
K3 = K.expand(3, 3, 3)

# the sentence of every kind of fault, after _blank()
SENTENCE = {
    "float": "<arg> must be a float tensor, got <x>",
    "mask": "<arg> must be a bool or uint8 tensor, got <x>",
    "depth_shape": "<arg> must be [B,#,H,W] or [B,H,W], non-empty, got <x>",
    "points_shape": "<arg> must be [B,#,H,W], non-empty, got <x>",
    "layout": "<arg> must be [B,#,H,W] or [B,N,#], got <x>",
    "map_shape": "<arg> <shape> is not [B,#,#,#] or [B,#,#]",
    "per_point": "<arg> <shape> does not hold one value for each of the <shape> coordinates of every image",
    "batch": "<arg> of # images for a batch of # (# or # expected)",
    "batch_exact": "<arg> of # images for a batch of #",
    "transform": "<arg> must be fp32 [#,#], [#,#,#] or [#,#,#]",
    "shape_pair": "<arg> must be (H, W)",
    "shape_positive": "<arg> must be positive, got <x>",
    "tol_number": "<arg> must be a number in fp32's range",
    "tol_range": "<arg> must be finite and not negative, got <x>",
    "too_many": "at most # images per call, got <x>",
}


def _blank(sentence, arg):
    """the sentence with its leading argument name, what follows ", got", the shapes and the numbers blanked (fp32 and uint8 stay)"""
    if arg:
        assert sentence.startswith(arg + " "), sentence
        sentence = "<arg>" + sentence[len(arg):]
    s = re.sub(r", got .*$", ", got <x>", sentence)
    return re.sub(r"(?<![A-Za-z0-9])\d+", "#", re.sub(r"\([\d, ]*\)", "<shape>", s))


def _tolerances(fn, arg, call):
    """the four ways a tolerance is wrong, for call(value)"""
    return [(fn, "tol_range", arg, lambda v=v: call(v)) for v in (-0.1, float("nan"), float("inf"))] + \
           [(fn, "tol_number", arg, lambda v=v: call(v)) for v in ("tol", 1e300)]


def _consistency(f):
    fn = f.__name__
    return [
        (fn, "float", "depth", lambda: f(ints, K, views, cams, T)),
        (fn, "float", "src_depths", lambda: f(depth, K, views.long(), cams, T)),
        (fn, "mask", "valid_in", lambda: f(depth, K, views, cams, T, valid_in=floats)),
        (fn, "mask", "src_masks", lambda: f(depth, K, views, cams, T, src_masks=views)),
        (fn, "depth_shape", "depth", lambda: f(torch.rand(B, 2, H, W), K, views, cams, T)),
        (fn, "map_shape", "valid_in", lambda: f(depth, K, views, cams, T, valid_in=bools[..., :3])),
        (fn, "batch_exact", "valid_in", lambda: f(depth, K, views, cams, T, valid_in=bools[:1])),
        (fn, "batch", "camera", lambda: f(depth, K3, views, cams, T)),
        (fn, "batch", "src_cameras[1]", lambda: f(depth, K, views, [K, K3], T)),
    ] + _tolerances(fn, "px_tol", lambda v: f(depth, K, views, cams, T, px_tol=v)) + _tolerances(fn, "rel_tol", lambda v: f(depth, K, views, cams, T, rel_tol=v))


def _normals_shared(f, first):
    """what normals_from_points (first = points) and normals_camera (first = depth, K) share"""
    fn = f.__name__
    return [
        (fn, "mask", "mask", lambda: f(*first, mask=floats)),
        (fn, "map_shape", "mask", lambda: f(*first, mask=bools[..., :3])),
        (fn, "map_shape", "mask", lambda: f(*first, mask=torch.ones(B, 2, H, W, dtype=torch.bool))),
        (fn, "batch", "mask", lambda: f(*first, mask=torch.ones(3, H, W, dtype=torch.bool))),
    ] + _tolerances(fn, "edge_rtol", lambda v: f(*first, edge_rtol=v))


wc, up, pc, rc = warp.warp_camera, unproject.unproject_camera, reproject.project_camera, reproject.render_depth_camera
ok = dict(depth=depth, camera=K, src_camera=K)
CASES = [
    ("gt_points", "float", "depth", lambda: gtpoints.gt_points(ints, K)),
    ("gt_points", "depth_shape", "depth", lambda: gtpoints.gt_points(torch.rand(B, 2, H, W), K)),
    ("gt_points", "depth_shape", "depth", lambda: gtpoints.gt_points(torch.rand(0, 1, H, W), K)),
    ("gt_points", "too_many", "", lambda: gtpoints.gt_points(torch.rand(MANY, 1, 1, 1), K)),
    ("gt_points", "batch", "camera", lambda: gtpoints.gt_points(depth, K3)),
    ("gt_points", "batch", "camera", lambda: gtpoints.gt_points(depth, cameras.Pinhole(K3))),
    ("gt_points", "batch_exact", "camera", lambda: gtpoints.gt_points(depth, cameras.BatchCamera([cameras.Pinhole(K)] * 3))),
    ("gt_points", "batch_exact", "camera", lambda: gtpoints.gt_points(depth, gtpoints.PreparedCamera(torch.zeros(3, 16), (1, 1, 1)))),

    ("unproject_camera", "float", "uv", lambda: up(uv.long(), K)),
    ("unproject_camera", "float", "depth", lambda: up(uv, K, depth=ints)),
    ("unproject_camera", "layout", "uv", lambda: up(torch.rand(B, 3, H, W), K)),
    ("unproject_camera", "layout", "uv", lambda: up(torch.rand(H, W), K)),
    ("unproject_camera", "batch", "uv", lambda: up(uv, K3)),
    ("unproject_camera", "batch_exact", "depth", lambda: up(uv[:1], K3, depth=depth)),
    ("unproject_camera", "shape_pair", "image_shape", lambda: up(uv, K, image_shape=(H,))),
    ("unproject_camera", "shape_pair", "image_shape", lambda: up(uv, K, image_shape="hw")),
    ("unproject_camera", "shape_positive", "image_shape", lambda: up(uv, K, image_shape=(0, W))),
    ("unproject_camera", "too_many", "", lambda: up(torch.rand(MANY, 1, 2), K)),
    ("get_rays", "too_many", "", lambda: unproject.get_rays(K, (MANY, H, W))),

    ("project_camera", "layout", "points", lambda: pc(torch.rand(B, 2, H, W), K)),
    ("project_camera", "layout", "points", lambda: pc(torch.rand(H, W), K)),
    ("project_camera", "shape_pair", "image_shape", lambda: pc(points, K, (H,))),
    ("project_camera", "shape_positive", "image_shape", lambda: pc(rows, K, (H, -1))),
    ("render_depth_camera", "layout", "points", lambda: rc(torch.rand(B, 2, H, W), K, (H, W))),
    ("render_depth_camera", "shape_pair", "image_shape", lambda: rc(points, K, None)),
    ("render_depth_camera", "shape_positive", "image_shape", lambda: rc(points, K, (0, 0))),

    ("remap", "float", "uv", lambda: remap.remap(src, uv.long())),
    ("remap", "mask", "src_mask", lambda: remap.remap(src, uv, src_mask=floats)),
    ("remap", "mask", "coord_valid", lambda: remap.remap(src, uv, coord_valid=floats)),
    ("remap", "layout", "uv", lambda: remap.remap(src, torch.rand(B, 3, H, W))),
    ("remap", "map_shape", "src_mask", lambda: remap.remap(src, uv, src_mask=bools[..., :3])),
    ("remap", "map_shape", "src_mask", lambda: remap.remap(src, uv, src_mask=torch.ones(H, W, dtype=torch.bool))),
    ("remap", "per_point", "coord_valid", lambda: remap.remap(src, uv, coord_valid=bools[..., :3])),
    ("remap", "batch", "src", lambda: remap.remap(src, uv3)),
    ("remap", "batch", "src_mask", lambda: remap.remap(src[:1], uv3, src_mask=bools)),
    ("remap", "batch", "coord_valid", lambda: remap.remap(src[:1], uv3, coord_valid=bools)),
    ("remap", "too_many", "", lambda: remap.remap(src[:1], torch.rand(MANY, 1, 2))),
    ("undistort", "shape_pair", "out_shape", lambda: remap.undistort(src, K, out_shape=(H,))),
    ("undistort", "shape_positive", "out_shape", lambda: remap.undistort(src, K, out_shape=(0, W))),
    ("undistort", "batch", "src", lambda: remap.undistort(src, K3)),

    ("warp_camera", "float", "depth", lambda: wc(src, depth=ints, camera=K, src_camera=K)),
    ("warp_camera", "float", "points", lambda: wc(src, points=points.long(), src_camera=K)),
    ("warp_camera", "float", "src_depth", lambda: wc(src, src_depth=ints, occlusion_tol=0.1, **ok)),
    ("warp_camera", "mask", "src_mask", lambda: wc(src, src_mask=floats, **ok)),
    ("warp_camera", "mask", "valid_in", lambda: wc(src, valid_in=floats, **ok)),
    ("warp_camera", "depth_shape", "depth", lambda: wc(src, depth=torch.rand(B, 2, H, W), camera=K, src_camera=K)),
    ("warp_camera", "points_shape", "points", lambda: wc(src, points=rows, src_camera=K)),
    ("warp_camera", "map_shape", "src_mask", lambda: wc(src, src_mask=bools[..., :3], **ok)),
    ("warp_camera", "map_shape", "valid_in", lambda: wc(src, valid_in=torch.ones(B, H * W, dtype=torch.bool), **ok)),
    ("warp_camera", "map_shape", "src_depth", lambda: wc(src, src_depth=torch.rand(B, 2, H, W), occlusion_tol=0.1, **ok)),
    ("warp_camera", "batch", "src", lambda: wc(torch.rand(3, 3, H, W), **ok)),
    ("warp_camera", "batch", "valid_in", lambda: wc(src, valid_in=torch.ones(3, H, W, dtype=torch.bool), **ok)),
    ("warp_camera", "batch", "src_camera", lambda: wc(src, depth=depth, camera=K, src_camera=K3)),
    ("warp_camera", "batch_exact", "camera", lambda: wc(src, depth=depth, camera=gtpoints.PreparedCamera(torch.zeros(1, 16), (1,)), src_camera=K)),
    ("warp_camera", "transform", "transform", lambda: wc(src, transform=torch.rand(3, 3), **ok)),
    ("warp_camera", "transform", "transform", lambda: wc(src, transform=torch.eye(4)[None].expand(3, 4, 4), **ok)),
    ("warp_camera", "transform", "transform", lambda: wc(src, transform=torch.eye(4).double(), **ok)),
    ("warp_camera", "too_many", "", lambda: wc(src[:1], depth=torch.rand(MANY, 1, 1, 1), camera=K, src_camera=K)),
    *_tolerances("warp_camera", "occlusion_tol", lambda v: wc(src, src_depth=floats, occlusion_tol=v, **ok)),

    ("normals_from_points", "float", "points", lambda: normals.normals_from_points(points.long())),
    ("normals_from_points", "float", "depth", lambda: normals.normals_from_points(points, depth=ints)),
    ("normals_from_points", "points_shape", "points", lambda: normals.normals_from_points(rows)),
    ("normals_from_points", "map_shape", "depth", lambda: normals.normals_from_points(points, depth=floats[..., :3])),
    ("normals_from_points", "batch_exact", "depth", lambda: normals.normals_from_points(points, depth=floats[:1])),
    ("normals_from_points", "too_many", "", lambda: normals.normals_from_points(torch.rand(MANY, 3, 1, 1))),
    *_normals_shared(normals.normals_from_points, (points,)),
    ("normals_camera", "float", "depth", lambda: normals.normals_camera(ints, K)),
    ("normals_camera", "depth_shape", "depth", lambda: normals.normals_camera(torch.rand(H, W), K)),
    ("normals_camera", "too_many", "", lambda: normals.normals_camera(torch.rand(MANY, 1, 1, 1), K)),
    *_normals_shared(normals.normals_camera, (depth, K)),

    *_consistency(consistency.depth_consistency),
    *_consistency(consistency.depth_consistency_composition),
]
FUNCTIONS = ("gt_points", "unproject_camera", "get_rays", "project_camera", "render_depth_camera", "remap", "undistort", "warp_camera",
             "normals_from_points", "normals_camera", "depth_consistency", "depth_consistency_composition")


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{fn}-{kind}-{arg or 'B'}-{k}" for k, (fn, kind, arg, _) in enumerate(CASES)])
def test_fault_is_reported_in_the_family_sentence(k):
    fn, kind, arg, call = CASES[k]
    with pytest.raises(ValueError) as e:
        call()
    msg = str(e.value)
    assert type(e.value) is ValueError and msg.startswith(fn + ": "), msg
    assert arg in msg, msg
    assert _blank(msg[len(fn) + 2:], arg) == SENTENCE[kind], msg


def test_table_covers_the_family():
    seen = {}
    for fn, kind, _, _ in CASES:
        seen.setdefault(fn, set()).add(kind)
    assert set(seen) == set(FUNCTIONS)
    assert {kind for kinds in seen.values() for kind in kinds} == set(SENTENCE)
    # every tolerance of the family is refused for a negative, a NaN, an infinite and a non-numeric value
    for fn in ("warp_camera", "normals_from_points", "normals_camera", "depth_consistency", "depth_consistency_composition"):
        assert {"tol_number", "tol_range"} <= seen[fn], fn


def test_views_transforms_and_shapes_keep_their_own_sentences():
    """the faults only one member of the family can report"""
    for f in (consistency.depth_consistency, consistency.depth_consistency_composition):
        fn = f.__name__
        with pytest.raises(ValueError, match=f"^{fn}: transforms must be fp32"):
            f(depth, K, views, cams, torch.eye(4))
        with pytest.raises(ValueError, match=f"^{fn}: src_depths: at most 255 views and {_lib.UD_RECON_MAX_B} image-view pairs"):
            f(depth, K, torch.rand(B, 129, 1, 1), [K] * 129, torch.eye(4).repeat(129, 1, 1))
    with pytest.raises(ValueError, match="^get_rays: shapes must be"):
        unproject.get_rays(K, (H,))
    with pytest.raises(ValueError, match="^project_camera: points must be an fp32 tensor"):
        pc(points.double(), K)


def test_tolerance_bits_are_those_of_the_fp32_rounding():
    """what the descriptors receive: the bit pattern of the value rounded to fp32, for the values the family's tests pass"""
    from unidepth_amd import _args
    for v, bits in ((0, 0), (0.0, 0), (1.0, 0x3F800000), (0.5, 0x3F000000), (0.25, 0x3E800000), (0.1, 0x3DCCCCCD), (0.01, 0x3C23D70A), (0.05, 0x3D4CCCCD),
                    (1e-50, 0)):
        val, got = _args.tolerance("f", "tol", v)
        assert got == bits == _args.f32_bits(float(v)) and val == torch.tensor(float(v), dtype=torch.float32).item(), (v, hex(got))
