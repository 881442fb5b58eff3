"""GPU parity of gt_points (unidepth_amd/gtpoints.py -> ud_reconstruct, csrc/reconstruct.hip) against the reference's own
Camera.reconstruct (tests/golden/gt_points.npz) at the bars measured by tools/make_golden_gt_points.py, and against that tool's numpy
fp32 restatement; guarded outputs, the per-image early exit, broadcasting, input layouts, camera objects, graph replay and
MetricsAccumulator.accumulate_metrics.  Every pixel of every case is compared: the generator keeps the residual maxima clear of
the exit threshold (tests/test_gt_points_cpu.py checks that without a GPU).  Shared helpers: tests/gt_points_common.py.

Every case runs once per process through the C-ABI with guarded buffers (_gpu_case) and is shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gt_points_common as cpu
import layout_guard as lg

gp = cpu.gp
pytestmark = pytest.mark.gpu

# Models whose kernel arithmetic has no libm call (only +, -, *, /, sqrt, all correctly rounded on both sides): bit-equal to the
# numpy fp32 restatement.  Spherical (sinf / cosf) and Fisheye624 (tanf) differ from numpy's functions in the last bits and keep the bar.
EXACT_MODELS = (gp.PINHOLE, gp.EUCM, gp.OPENCV, gp.MEI)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_as_numpy(out, want):
    """bit-equal to a numpy result; where both are NaN the payload is not compared (the host's and the device's default NaN differ)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(out), nan) and np.array_equal(_bits(np.where(nan, 0, out).astype(np.float32)), _bits(np.where(nan, 0, want).astype(np.float32)))


def _raw_call(depth, params, models):
    """ud_reconstruct with `points` and `work` inside sentinel-filled allocations; returns the points (numpy) after checking the guards."""
    from unidepth_amd import _lib
    from unidepth_amd.ops import cur_stream
    B, _, H, W = depth.shape
    n_iter = sum(m in gp.ITERATIVE for m in models)
    nbytes = int(_lib.lib.ud_reconstruct_work_bytes(B, H, W, n_iter))
    d = torch.from_numpy(depth).cuda()
    p = torch.from_numpy(params).cuda()
    pts = lg.guarded(B * 3, H * W, H * W, torch.float32)
    guards = [pts]
    desc = _lib.UdReconstruct()
    desc.depth, desc.params, desc.points = d.data_ptr(), p.data_ptr(), pts.ptr()
    desc.B, desc.H, desc.W = B, H, W
    if nbytes:
        assert nbytes % 16 == 0
        work = lg.guarded(1, nbytes // 4, nbytes // 4, torch.float32, pre_rows=4, post_rows=4)
        assert work.ptr() % 16 == 0
        desc.work, desc.work_bytes = work.ptr(), nbytes
        guards.append(work)
    for b, m in enumerate(models):
        desc.model[b] = m
    _lib.check(_lib.lib.ud_reconstruct(C.byref(desc), cur_stream()), "ud_reconstruct")
    torch.cuda.synchronize()
    lg.check_guards(*guards)
    return pts.view.reshape(B, 3, H, W).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    c = cpu.case(name)
    return _raw_call(c["depth"], c["params"], c["models"])


def _camera(name):
    from unidepth_amd import cameras
    return gp.case_camera(cameras, name)


def _points(depth, camera):
    from unidepth_amd import gtpoints
    out = gtpoints.gt_points(depth, camera)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    return out


@pytest.mark.parametrize("name", list(gp.CASES))
def test_case_against_reference_and_restatement(name):
    """every point of every stored case: the reference's output at the measured bar, NaN positions exact, guards intact; against the
    fp32 restatement bit for bit for the models without a libm call, at the bar for the others"""
    c = cpu.case(name)
    out = _gpu_case(name)                                       # raises if a guard element of points or work was rewritten
    ref = np.load(gp.GOLDEN)[name + ".out"]
    bars = cpu.bars()
    w_ref = cpu.assert_within_bars(out, ref, c, bars, f"{name} vs reference")
    w_r32 = cpu.assert_within_bars(out, c["r32"], c, bars, f"{name} vs fp32 restatement")
    e = gp.error_ratio(out.astype(np.float64) - c["r32"].astype(np.float64), c["r64"], c["depth"])
    per_model = {}
    for b, m in enumerate(c["models"]):
        per_model[gp.MODEL_NAMES[m]] = max(per_model.get(gp.MODEL_NAMES[m], 0.0), float(e[b].max()))
        if m in EXACT_MODELS:
            assert _same_as_numpy(out[b], c["r32"][b]), f"{name}: image {b} ({gp.MODEL_NAMES[m]}) is not bit-equal to the restatement"
    print(f"{name}: {w_ref:.3f} of the bar against the reference, {w_r32:.3f} against the restatement; largest difference from the restatement "
          + ", ".join(f"{k} {v:.3e}" for k, v in per_model.items()))
    # the Python surface gives the same bits as the raw call
    got = _points(torch.from_numpy(c["depth"]).cuda(), _camera(name)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(out))


def test_early_exit_is_per_image():
    """the weakly distorted OPENCV image alone (B = 1), beside the strongly distorted one, and with the two in the other order: the same
    bits.  One shared row of residual maxima would keep the weak image iterating as long as the strong one."""
    c = cpu.case("opencv_37x53_b2_iters")
    assert c["info"]["steps"][0] < c["info"]["steps"][1]
    both = _gpu_case("opencv_37x53_b2_iters")
    for b in (0, 1):
        alone = _raw_call(c["depth"][b:b + 1], c["params"][b:b + 1], [c["models"][b]])
        assert np.array_equal(_bits(alone[0]), _bits(both[b])), f"image {b} alone differs from image {b} in the batch"
    swapped = _raw_call(c["depth"][::-1].copy(), c["params"][::-1].copy(), c["models"][::-1])
    assert np.array_equal(_bits(swapped[::-1]), _bits(both))


def test_single_iterative_camera_broadcasts_over_the_batch():
    from unidepth_amd import cameras
    name = "broadcast_opencv_9x29_b3"
    depth, params, models = gp.case_inputs(name)
    assert params.shape[0] == 1 and depth.shape[0] == 3
    cam = _camera(name)
    assert isinstance(cam, cameras.OPENCV)
    d = torch.from_numpy(depth).cuda()
    whole = _points(d, cam)
    assert np.array_equal(_bits(whole.cpu().numpy()), _bits(_gpu_case(name)))
    for b in range(3):
        assert torch.equal(_points(d[b:b + 1], cam).view(torch.int32), whole[b:b + 1].view(torch.int32))
    # a closed-form camera with one row broadcasts the same way, and B rows are taken row by row
    depth2, params2, _ = gp.case_inputs("eucm_9x29_b2")
    d2 = torch.from_numpy(depth2).cuda()
    one = cameras.EUCM(torch.from_numpy(params2[:1, :6]))
    both = cameras.EUCM(torch.from_numpy(params2[:, :6]))
    assert torch.equal(_points(d2, one)[1].view(torch.int32), _points(d2[1:], one)[0].view(torch.int32))
    assert np.array_equal(_bits(_points(d2, both).cpu().numpy()), _bits(_gpu_case("eucm_9x29_b2")))


def test_depth_layouts_and_dtypes():
    name = "mixed_37x53_b6"
    c = cpu.case(name)
    cam = _camera(name)
    d = torch.from_numpy(c["depth"]).cuda()
    want = torch.from_numpy(_gpu_case(name)).cuda().view(torch.int32)
    assert torch.equal(_points(d[:, 0], cam).view(torch.int32), want)                       # [B,H,W]
    t = d[:, 0].permute(0, 2, 1).contiguous().permute(0, 2, 1)                              # a transposed view of the same values
    assert not t.is_contiguous() and torch.equal(_points(t, cam).view(torch.int32), want)
    wide = torch.full((6, 1, 37, 60), 3.0, device="cuda")
    wide[..., 4:57] = d
    assert torch.equal(_points(wide[..., 4:57], cam).view(torch.int32), want)               # a column window of a wider buffer
    assert torch.equal(_points(d.double(), cam).view(torch.int32), want)                    # fp64 of fp32 values converts back exactly
    h = d.half()
    assert torch.equal(_points(h, cam).view(torch.int32), _points(h.float().contiguous(), cam).view(torch.int32))
    assert torch.equal(_points(d.bfloat16(), cam).view(torch.int32), _points(d.bfloat16().float(), cam).view(torch.int32))


def test_camera_objects():
    """intrinsics tensors, own classes, stand-ins for the reference's classes (matched by class name and .params), Camera.reconstruct
    and add_points give gt_points' bits; the camera is not modified"""
    from unidepth_amd import cameras, gtpoints
    name = "mixed_5x7_b6"
    c = cpu.case(name)
    d = torch.from_numpy(c["depth"]).cuda()
    want = torch.from_numpy(_gpu_case(name)).cuda().view(torch.int32)

    def standin(model, row):
        cls = type(gp.MODEL_NAMES[model], (), {})
        o = cls()
        o.params = torch.from_numpy(row[: gp.N_PARAMS[model]].copy())[None]
        return o
    members = [standin(m, r) for m, r in zip(c["models"], c["params"])]
    wrapper = type("BatchCamera", (), {})()
    wrapper.cameras = [members[:2], members[2:]]                                        # nested lists flatten
    assert torch.equal(_points(d, wrapper).view(torch.int32), want)
    own = _camera(name)
    before = own.params.clone()
    assert torch.equal(own.reconstruct(d).view(torch.int32), want)
    assert torch.equal(own.params, before)
    for b, member in enumerate(own.cameras):                                             # every class has reconstruct
        assert torch.equal(member.reconstruct(d[b:b + 1]).view(torch.int32), want[b:b + 1])
    prepared = gtpoints.prepare_camera(own, 6, "cuda")
    assert prepared.params.is_cuda and prepared.models == tuple(c["models"])
    assert torch.equal(_points(d, prepared).view(torch.int32), want)
    inputs = {"depth": d, "camera": cameras.Pinhole(params=torch.tensor([[1.0, 1.0, 0.0, 0.0]])), "camera_original": own}
    assert gtpoints.add_points(inputs) is inputs and torch.equal(inputs["points"].view(torch.int32), want)
    # an intrinsics tensor is the Pinhole of its fx, fy, cx, cy; on the host or on the device, one matrix or one per image
    pd, pp, _ = gp.case_inputs("pinhole_5x7_b2")
    K = torch.zeros(2, 3, 3)
    for (r, col), i in (((0, 0), 0), ((1, 1), 1), ((0, 2), 2), ((1, 2), 3)):
        K[:, r, col] = torch.from_numpy(pp[:, i])
    K[:, 2, 2] = 1.0
    dd = torch.from_numpy(pd).cuda()
    pin = torch.from_numpy(_gpu_case("pinhole_5x7_b2")).cuda().view(torch.int32)
    for Kt in (K, K.cuda(), K.double()):
        assert torch.equal(_points(dd, Kt).view(torch.int32), pin)
    assert torch.equal(_points(dd, K[1]).view(torch.int32)[1], pin[1])
    skew = K.clone()
    skew[1, 0, 1] = 0.25                                                                # on the device there is no read-back: that image is NaN
    got = _points(dd, skew.cuda())
    assert torch.equal(got[0].view(torch.int32), pin[0]) and bool(torch.isnan(got[1]).all())
    with pytest.raises(ValueError, match="skew"):
        _points(dd, skew)
    assert torch.equal(_points(dd, cameras.Pinhole(K)).view(torch.int32), pin)
    del inputs["points"]
    inputs.pop("camera_original")
    inputs["camera"], inputs["depth"] = K, dd
    assert torch.equal(gtpoints.add_points(inputs)["points"].view(torch.int32), pin)


def _captured(depth, cam):
    """gt_points(depth, cam) captured once on static buffers: (graph, static output)"""
    from unidepth_amd import gtpoints
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _points(depth, cam)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gtpoints.gt_points(depth, cam)
    return graph, out


def test_graph_replay_with_changed_depth():
    """the mixed B = 6 batch captured once and replayed twice with a changed depth: each replay equals the eager call bitwise"""
    from unidepth_amd import gtpoints
    name = "mixed_37x53_b6"
    c = cpu.case(name)
    cam = gtpoints.prepare_camera(_camera(name), 6, "cuda")                                  # uploaded before the capture
    d0 = torch.from_numpy(c["depth"]).cuda()
    static = d0.clone()
    graph, out = _captured(static, cam)
    g = torch.Generator().manual_seed(77)
    for k in range(2):
        new = (d0 * (0.5 + torch.rand(d0.shape, generator=g).cuda())).contiguous()
        new[k, 0, 3, 5] = float("nan")
        static.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = _points(new, cam)
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), f"replay {k} differs from the eager call"
    static.copy_(d0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(_gpu_case(name)))


def test_graph_replay_clears_the_residual_maxima():
    """The residual maxima depend on the camera rows alone, so the replays change THOSE: the weakly and the strongly distorted OPENCV
    camera captured in one order, then their rows swapped in the static parameter tensor.  The maxima only grow (atomicMax): without
    the call's own clear the strong camera's maxima of the first run would keep the weak image, now in its place, iterating, and extra
    trust-region steps change its bits."""
    from unidepth_amd import gtpoints
    name = "opencv_37x53_b2_iters"
    c = cpu.case(name)
    assert c["info"]["steps"][0] < c["info"]["steps"][1]
    cam = gtpoints.prepare_camera(_camera(name), 2, "cuda")
    rows = cam.params.clone()
    depth = torch.from_numpy(c["depth"]).cuda()
    graph, out = _captured(depth, cam)
    want = torch.from_numpy(_gpu_case(name)).cuda()
    for k in range(4):                                                                       # orders: swapped, original, swapped, original
        order = [1, 0] if k % 2 == 0 else [0, 1]
        cam.params.copy_(rows[order])
        graph.replay()
        torch.cuda.synchronize()
        for b in (0, 1):                                                                     # image b now has camera order[b] on depth b
            alone = _points(depth[b:b + 1], gtpoints.PreparedCamera(rows[order[b]:order[b] + 1].contiguous(), cam.models[:1]))
            assert torch.equal(out[b:b + 1].view(torch.int32), alone.view(torch.int32)), f"replay {k}: image {b} differs from the eager call"
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_accumulate_metrics():
    """the reference's accumulate_metrics on a 37 x 53 batch: depth, depth_mask, camera_original and predictions {"depth", "points"}
    equal accumulate_depth plus accumulate_3d fed with gt_points; the keys carry the reference's names"""
    from unidepth_amd import cameras, eval_ops, gtpoints
    name = "mixed_37x53_b6"
    c = cpu.case(name)
    cam = _camera(name)
    depth = torch.from_numpy(c["depth"]).cuda()
    mask = torch.isfinite(depth) & (depth > 1e-3)
    g = torch.Generator().manual_seed(78)
    gt_pts = gtpoints.gt_points(depth, cam)
    pred_depth = (torch.nan_to_num(depth, nan=1.0).clamp_min(0.1) * (0.9 + 0.2 * torch.rand(depth.shape, generator=g).cuda())).contiguous()
    pred_pts = (torch.nan_to_num(gt_pts, nan=0.0) * 1.03 + 0.05 * (torch.rand(gt_pts.shape, generator=g).cuda() - 0.5)).contiguous()
    wrong = cameras.Pinhole(params=torch.tensor([[10.0, 10.0, 1.0, 1.0]]))                   # camera_original wins over camera

    def inputs():
        return {"depth": depth, "depth_mask": mask, "camera": wrong, "camera_original": cam}

    acc = eval_ops.MetricsAccumulator(0.01, 80.0)
    inp = inputs()
    acc.accumulate_metrics(inp, {"depth": pred_depth, "points": pred_pts})
    assert "points" not in inputs() and torch.equal(inp["points"].view(torch.int32), gt_pts.view(torch.int32))
    got = acc.get_evaluation()
    want_acc = eval_ops.MetricsAccumulator(0.01, 80.0)
    want_acc.accumulate_depth(depth, pred_depth, mask)
    want_acc.accumulate_3d(gt_pts, pred_pts, mask)
    want = want_acc.get_evaluation()
    assert list(got) == list(want) and set(eval_ops.EVAL_3D_KEYS) <= set(got) and "d1" in got
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])
    assert np.isfinite(got["F1"]) and np.isfinite(got["chamfer"]) and got["chamfer"] > 0
    # no points in the predictions: depth keys only; named predictions carry the reference's names; points_mask is preferred
    acc.accumulate_metrics(inputs(), {"depth": pred_depth})
    only = acc.get_evaluation()
    assert not set(eval_ops.EVAL_3D_KEYS) & set(only) and only["d1"] == want["d1"]
    pm = mask & (depth < 15.0)
    inp = inputs()
    inp["points_mask"] = pm
    acc.accumulate_metrics(inp, {"depth-lr": pred_depth, "points_lr": pred_pts, "confidence": pred_depth})
    named = acc.get_evaluation()
    want_acc.accumulate_depth(depth, pred_depth, mask, name="lr")
    want_acc.accumulate_3d(gt_pts, pred_pts, pm, name="lr")
    assert named == want_acc.get_evaluation() and "lr_d1" in named and "lr_F1" in named
    # keyframe_idx: that image alone
    acc.accumulate_metrics(inputs(), {"depth": pred_depth, "points": pred_pts}, keyframe_idx=2)
    want_acc.accumulate_depth(depth[2:3], pred_depth[2:3], mask[2:3])
    want_acc.accumulate_3d(gt_pts[2:3], pred_pts[2:3], mask[2:3])
    assert acc.get_evaluation() == want_acc.get_evaluation()
