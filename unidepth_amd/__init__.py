"""unidepth_amd -- MI355X (gfx950) native engine for the UniDepth `infer()` paths (UniDepthV2 on DINOv2 ViT-S/B/L; UniDepthV1 on ConvNeXt-L).

Public surface mirrors the reference (lpiccinelli-eth/UniDepth, unidepth/models/__init__.py):
    from unidepth_amd import UniDepthV2
    model = UniDepthV2.from_pretrained(dir_or_repo).to("cuda").eval(); out = model.infer(rgb, camera)
All device arithmetic runs in libunidepth_hip.so (hand-written HIP); importing this package without the
built library raises ImportError -- there is no CPU / eager-PyTorch fallback."""
from . import _lib  # noqa: F401  (fails loudly when the HIP library is missing)

_POINTCLOUD = ("PointCloud", "pack_points", "from_prediction", "get_pointcloud_from_rgbd", "save_ply", "save_file_ply")
_MATCHING = ("match_gt", "match_intrinsics")
_VISUALIZATION = ("colorize", "colorize_batch", "demo_panel", "image_grid", "save_png", "preload_colormap")
_REPROJECT = ("RenderedView", "render_depth", "reproject", "project_points", "downsample", "render_depth_camera", "project_camera")
_TESTPREP = ("TestGeometry", "test_geometry", "prepare_test_batch", "resize_aa", "original_image")
_GTPOINTS = ("gt_points", "add_points", "prepare_camera")
_UNPROJECT = ("unproject_camera", "get_rays")
_REMAP = ("remap", "undistort", "overlap_mask")
_WARP = ("warp_camera",)
_NORMALS = ("normals_from_points", "normals_camera", "eval_normals")
_CONSISTENCY = ("depth_consistency", "depth_consistency_composition", "invert_rigid")
_TSDF = ("TsdfVolume", "tsdf_integrate", "tsdf_integrate_composition", "tsdf_points", "tsdf_render", "tsdf_render_composition")
_TSDFMESH = ("TriangleMesh", "tsdf_mesh", "tsdf_mesh_composition", "save_mesh_ply")
_ICP = ("icp_linearize", "icp_linearize_composition", "icp_solve", "track_camera", "track_camera_composition")
_PYRAMID = ("DepthFilter", "prepare_depth_filter", "depth_pyramid", "depth_pyramid_composition", "pyramid_cameras", "track_camera_pyramid")
__all__ = ["UniDepthV2", "UniDepthV1", "UniDepth", *_POINTCLOUD, *_MATCHING, *_VISUALIZATION, *_REPROJECT, *_TESTPREP, *_GTPOINTS, *_UNPROJECT, *_REMAP, *_WARP, *_NORMALS,
           *_CONSISTENCY, *_TSDF, *_TSDFMESH, *_ICP, *_PYRAMID]


def __getattr__(name):
    if name == "UniDepthV2":
        from .unidepthv2 import UniDepthV2
        return UniDepthV2
    if name in ("UniDepthV1", "UniDepth"):            # hubconf-style entry point / the V1 family (ConvNeXt-L / ViT-L)
        from . import hub
        return getattr(hub, name)
    if name in _POINTCLOUD:                           # packed point clouds from infer() outputs (pointcloud.py, csrc/pointcloud.hip)
        from . import pointcloud
        return getattr(pointcloud, name)
    if name in _MATCHING:                             # outputs matched to the ground truth (matching.py, csrc/matchgt.hip)
        from . import matching
        return getattr(matching, name)
    if name in _VISUALIZATION:                        # depth maps as colour images (visualization.py, csrc/colorize.hip)
        from . import visualization
        return getattr(visualization, name)
    if name in _REPROJECT:                            # point clouds back into depth maps (reproject.py, csrc/splat.hip, csrc/project.hip)
        import importlib                              # not `from . import reproject`: that asks this function for "reproject" first
        return getattr(importlib.import_module(".reproject", __name__), name)
    if name in _TESTPREP:                             # validation inputs from raw uint8 images (testprep.py, csrc/testprep.hip)
        from . import testprep
        return getattr(testprep, name)
    if name in _GTPOINTS:                             # ground-truth point maps for the validation loop (gtpoints.py, csrc/reconstruct.hip)
        from . import gtpoints
        return getattr(gtpoints, name)
    if name in _UNPROJECT:                            # rays at arbitrary image coordinates (unproject.py, csrc/unproject.hip)
        from . import unproject
        return getattr(unproject, name)
    if name in _REMAP:                                # maps sampled at arbitrary image coordinates (remap.py, csrc/remap.hip)
        import importlib                              # not `from . import remap`: that asks this function for "remap" first
        return getattr(importlib.import_module(".remap", __name__), name)
    if name in _WARP:                                 # backward warping through the camera models in one launch (warp.py, csrc/warp.hip)
        from . import warp
        return getattr(warp, name)
    if name in _NORMALS:                              # surface normals from points or depth, and their metrics (normals.py, csrc/normals.hip)
        from . import normals
        return getattr(normals, name)
    if name in _CONSISTENCY:                          # multi-view depth check and fusion in one launch (consistency.py, csrc/consistency.hip)
        from . import consistency
        return getattr(consistency, name)
    if name in _TSDF:                                 # depth views fused into a TSDF volume, and its surface as points (tsdf.py, csrc/tsdf.hip)
        from . import tsdf
        return getattr(tsdf, name)
    if name in _TSDFMESH:                             # a TSDF volume's surface as a triangle mesh (tsdfmesh.py, csrc/tsdf_mesh.hip)
        from . import tsdfmesh
        return getattr(tsdfmesh, name)
    if name in _ICP:                                  # camera tracking against a model view: point-to-plane ICP (icp.py, csrc/icp.hip)
        from . import icp
        return getattr(icp, name)
    if name in _PYRAMID:                              # depth filter, pyramid and coarse-to-fine tracking (pyramid.py, csrc/pyramid.hip)
        from . import pyramid
        return getattr(pyramid, name)
    raise AttributeError(name)
