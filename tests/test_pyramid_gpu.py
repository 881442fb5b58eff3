"""GPU parity of depth_pyramid, pyramid_cameras, track_camera_pyramid and TsdfVolume.track_pyramid (unidepth_amd/pyramid.py ->
ud_depth_pyramid, csrc/pyramid.hip).  The pyramid has two oracles, both bit for bit at every level, in depth and weights: the numpy fp32
restatement of csrc/pyramid_point.h (tests/pyramid_common.py, which tests/test_pyramid_cpu.py holds against the host build of the header)
and depth_pyramid_composition, the same definition in vectorised torch.  The level cameras are held to the identities that define them;
track_camera_pyramid to the chain it is by definition, spelled out here with depth_pyramid, pyramid_cameras and track_camera; and
TsdfVolume.track_pyramid to the pose the single-level track reaches on the fused corner of tests/test_icp_gpu.py."""
import functools
import math

import numpy as np
import pytest
import torch

import icp_common as ic
import layout_guard as lg
import pyramid_common as pc
import tsdf_common as tc
from host_program import assert_same

pytestmark = pytest.mark.gpu
F = np.float32
TILES = (1, 2)                                                       # 32 x 32 and 64 x 16


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def _filter(radius, sigma_range=pc.SIGMA_RANGE):
    from unidepth_amd import pyramid
    return None if radius == 0 else pyramid.prepare_depth_filter(radius, pc.SIGMA_SPACE, sigma_range, "cuda")


def _restated(s, levels, radius, use_mask, use_w, gate, sigma_range=pc.SIGMA_RANGE):
    kw = dict(radius=radius)
    if radius:
        ws, wr, inv_bin = pc.tables(radius, pc.SIGMA_SPACE, sigma_range)
        kw.update(ws=ws, wr=wr, inv_bin=inv_bin)
    return pc.restate(s["depth"], levels, mask=s["mask"] if use_mask else None, weights=s["weights"] if use_w else None, gate=gate, **kw)


def _flat(res, B):
    """depth_pyramid's result as one tuple of [B,1,h,w] tensors (depth levels, then weight levels) with their names"""
    d, w = res if isinstance(res, tuple) else (res, None)
    maps = list(d) + list(w or ())
    names = [f"depth[{l}]" for l in range(len(d))] + [f"weights[{l}]" for l in range(len(w or ()))]
    return tuple(m.reshape(B, 1, *m.shape[-2:]) for m in maps), names


def _check(s, levels, radius, use_mask, use_w, gate, what, sigma_range=pc.SIGMA_RANGE, composition=True):
    """the fused kernel with both tile shapes against the restatement and the composition"""
    from unidepth_amd import pyramid
    B = s["depth"].shape[0]
    kw = dict(mask=_dev(s["mask"]) if use_mask else None, weights=_dev(s["weights"]) if use_w else None, filter=_filter(radius, sigma_range), gate=gate)
    depth = _dev(s["depth"])
    rd, rw = _restated(s, levels, radius, use_mask, use_w, gate, sigma_range)
    want = tuple(_dev(x)[:, None] for x in rd + (rw or []))
    for tile in TILES:
        pyramid._LAUNCH_OPTIONS["tile"] = tile
        try:
            got, names = _flat(pyramid.depth_pyramid(depth, levels, **kw), B)
        finally:
            pyramid._LAUNCH_OPTIONS["tile"] = 0
        assert len(got) == levels * (2 if use_w else 1)
        assert_same(got, want, names, f"{what} tile {tile} against the restatement")
    if composition:
        comp, _ = _flat(pyramid.depth_pyramid_composition(depth, levels, **kw), B)
        assert_same(comp, want, names, f"{what}: the composition against the restatement")


SIZES = ((1, 1, 1), (2, 2, 2), (8, 8, 4), (33, 65, 3), (67, 129, 3), (31, 97, 3), (64, 64, 4))


@pytest.mark.parametrize("H,W,levels", SIZES)
@pytest.mark.parametrize("radius", (0, 1, 4))
def test_pyramid_against_restatement_and_composition(H, W, levels, radius):
    """B = 3, two scenes: everything on with a finite gate, everything off with an infinite one, and each optional input alone"""
    for seed in (0, 1):
        s = pc.scene(3, H, W, seed)
        for use_mask, use_w, gate in ((1, 1, pc.GATE), (0, 0, math.inf)) + (((1, 0, math.inf), (0, 1, pc.GATE)) if seed == 0 else ()):
            _check(s, levels, radius, use_mask, use_w, gate, f"{H}x{W} L={levels} r={radius} seed={seed} mask={use_mask} w={use_w}")


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257))
def test_single_rows_and_columns(n):
    """1 x N and N x 1 images (one level: nothing to halve) around the tile widths and the workgroup size, r = 4: every tap above and
    below (or left and right) lies outside the image"""
    for H, W in ((1, n), (n, 1)):
        _check(pc.scene(2, H, W, seed=n), 1, 4, 1, 1, math.inf, f"{H}x{W}")
        _check(pc.scene(2, H, W, seed=n), 1, 0, 0, 0, math.inf, f"{H}x{W} r=0", composition=False)
    _check(pc.scene(2, 2, n, seed=n), 2, 1, 1, 1, pc.GATE, f"2x{n}")


def test_largest_batch():
    _check(pc.scene(256, 4, 4, seed=3), 3, 1, 1, 1, pc.GATE, "B=256 4x4")


@pytest.mark.parametrize("radius", (0, 1, 4))
def test_special_values(radius):
    """NaN, +-inf, negatives, -0, subnormals and a delta * inv_bin that overflows: the bits of the restatement, and no NaN anywhere"""
    from unidepth_amd import pyramid
    s = pc.special_scene()
    for gate in (math.inf, 0.0, 0.5):
        _check(s, 3, radius, 1, 1, gate, f"special r={radius} gate={gate}", sigma_range=1e-3)
    d, w = pyramid.depth_pyramid(_dev(s["depth"]), 3, mask=_dev(s["mask"]), weights=_dev(s["weights"]), filter=_filter(radius, 1e-3))
    assert not any(bool(torch.isnan(x).any()) for x in d + w)


def test_prepared_filter_tables():
    from unidepth_amd import pyramid
    f = pyramid.prepare_depth_filter(2, 1.5, 0.05, "cuda")
    ws, wr, inv_bin = pc.tables(2, 1.5, 0.05)
    assert f.radius == 2 and f.ws.is_cuda and f.wr.is_cuda and f.ws.dtype == f.wr.dtype == torch.float32
    assert pc.same_bits(f.ws.cpu().numpy(), ws) and pc.same_bits(f.wr.cpu().numpy(), wr) and f.inv_bin_bits == pc.f32_bits(float(inv_bin))


# ---- the C-ABI on guarded allocations ------------------------------------------------------------------------------------------------

def _odd(t):
    """a copy of t whose first element sits at an odd element offset of its allocation"""
    buf = torch.empty(t.numel() + 3, device="cuda", dtype=t.dtype)
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1))
    return v


@pytest.mark.parametrize("tile", TILES)
def test_c_abi_guarded_outputs_and_absent_levels(tile):
    """the raw call with every input at an odd element offset (the mask at an odd byte) and every output a guarded allocation at an odd
    offset: the bits of the restatement, no guard element rewritten; then with out_depth[1] and out_weights[0] absent: the others
    unchanged, nothing else written"""
    import ctypes as C
    from unidepth_amd import _lib
    from unidepth_amd.ops import cur_stream
    B, H, W, L, r = 2, 33, 65, 3, 2
    s = pc.scene(B, H, W, seed=5)
    f = _filter(r)
    depth, mask, weights = _odd(_dev(s["depth"])), _odd(_dev(s["mask"])), _odd(_dev(s["weights"]))
    ws, wr = _odd(f.ws), _odd(f.wr)
    assert depth.data_ptr() % 8 == 4 and mask.data_ptr() % 2 == 1
    rd, rw = _restated(s, L, r, 1, 1, pc.GATE)
    sizes = pc.level_sizes(H, W, L)
    for absent_d, absent_w in ((), ()), ((1,), (0,)):
        gd = [lg.guarded(1, B * h * w, B * h * w + 3, torch.float32, pre_rows=2, post_rows=2, offset_cols=1) for h, w in sizes]
        gw = [lg.guarded(1, B * h * w, B * h * w + 3, torch.float32, pre_rows=2, post_rows=2, offset_cols=1) for h, w in sizes]
        desc = _lib.UdDepthPyramid()
        desc.depth, desc.mask, desc.weights, desc.ws, desc.wr = depth.data_ptr(), mask.data_ptr(), weights.data_ptr(), ws.data_ptr(), wr.data_ptr()
        desc.B, desc.H, desc.W, desc.levels, desc.radius, desc.tile = B, H, W, L, r, tile
        desc.gate_bits, desc.inv_bin_bits = pc.f32_bits(pc.GATE), f.inv_bin_bits
        for l in range(L):
            desc.out_depth[l] = None if l in absent_d else gd[l].ptr()
            desc.out_weights[l] = None if l in absent_w else gw[l].ptr()
        assert _lib.lib.ud_depth_pyramid(C.byref(desc), cur_stream()) == 0, _lib.lib.ud_last_error()
        torch.cuda.synchronize()
        lg.check_guards(*gd, *gw)
        for l in range(L):
            for g, want, absent, name in ((gd[l], rd[l], absent_d, "depth"), (gw[l], rw[l], absent_w, "weights")):
                if l in absent:                                      # never written: the sentinel still fills the view
                    assert bool((g.view.view(torch.int32) == lg.SENTINEL[torch.float32]).all()), (name, l)
                else:
                    assert pc.same_bits(g.view.cpu().numpy().reshape(want.shape), want), (name, l, absent_d, absent_w)


def test_graph_replay_with_a_rewritten_depth():
    """depth_pyramid captured once; replayed after the depth, the mask and the weights were rewritten in place: each replay equals the
    restatement of what the buffers hold"""
    from unidepth_amd import pyramid
    B, H, W, L = 2, 33, 65, 3
    a, b = pc.scene(B, H, W, seed=0), pc.scene(B, H, W, seed=9)
    depth, mask, weights = _dev(a["depth"]).clone(), _dev(a["mask"]).clone(), _dev(a["weights"]).clone()
    f = _filter(2)
    fn = lambda: pyramid.depth_pyramid(depth, L, mask=mask, weights=weights, filter=f, gate=pc.GATE)        # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    for k in range(3):
        s = b if k % 2 == 0 else a
        depth.copy_(_dev(s["depth"])), mask.copy_(_dev(s["mask"])), weights.copy_(_dev(s["weights"]))
        graph.replay()
        torch.cuda.synchronize()
        rd, rw = _restated(s, L, 2, 1, 1, pc.GATE)
        got, names = _flat(static, B)
        assert_same(got, tuple(_dev(x)[:, None] for x in rd + rw), names, f"replay {k}")


# ---- the level cameras ---------------------------------------------------------------------------------------------------------------

def test_level_cameras_on_the_device():
    """all six models in one batch: project_camera through level l gives the level-0 coordinates times 2^-l, and unproject_camera on
    [B,N,2] rows at level l gives level 0 at the rows times 2^l, bit for bit (rows: the iterative models leave their loop on the maximum
    over the same set of coordinates on both sides)"""
    from unidepth_amd import pyramid
    from unidepth_amd.reproject import project_camera
    from unidepth_amd.unproject import unproject_camera
    H, W, f, L = 96, 128, 70.0, 4
    models = ic.MODELS
    B = len(models)
    cam = ic.prepared(np.stack([tc.row_for(m, H, W, f) for m in models]), models)
    cams = pyramid.pyramid_cameras(cam, B, L, "cuda")
    assert len(cams) == L and cams[0].params.data_ptr() == cam.params.data_ptr() and all(c.models == cam.models and c.params.shape == (B, 16) for c in cams)
    g = np.random.RandomState(31)
    xyz = _dev(np.stack([g.uniform(-0.8, 0.8, (B, 500)), g.uniform(-0.6, 0.6, (B, 500)), g.uniform(1.0, 3.0, (B, 500))], axis=-1).astype(F))
    uv0, inside0, _ = project_camera(xyz, cams[0], (H, W))
    assert bool(inside0.float().mean() > 0.5)
    rows0 = _dev(np.stack([g.uniform(2, W - 2, (B, 300)), g.uniform(2, H - 2, (B, 300))], axis=-1).astype(F))
    for l in range(1, L):
        uvl, _, _ = project_camera(xyz, cams[l], (H >> l, W >> l))
        assert_same((uvl,), (uv0 * 0.5 ** l,), ("uv",), f"project level {l}")
        rows_l = rows0 * 0.5 ** l
        assert torch.equal(rows_l * 2.0 ** l, rows0)
        assert_same((unproject_camera(rows_l, cams[l]),), (unproject_camera(rows0, cams[0]),), ("rays",), f"unproject level {l}")
    # a camera given as an object or a tensor goes through prepare_camera; a level count of 1 is that camera alone
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    one = pyramid.pyramid_cameras(K, 2, 2, "cuda")
    assert one[1].params[:, :4].tolist() == [[f / 2, f / 2, W / 4, H / 4]] * 2 and len(pyramid.pyramid_cameras(K, 2, 1, "cuda")) == 1


# ---- track_camera_pyramid ------------------------------------------------------------------------------------------------------------

def _track_case(frame_models, model_models, L, seed=0):
    """a frame of 37 x 53 against model maps of 48 x 64 and its halvings (icp_common.mixed_case at every level's size)"""
    cases = [ic.mixed_case(frame_models, model_models, H=37, W=53, Hm=48 >> l, Wm=64 >> l, seed=seed) for l in range(L)]
    c = cases[0]
    levels = [(_dev(k["mp"]), _dev(k["mn"]), _dev(k["mv"]), ic.prepared(k["params_model"], k["models_model"])) for k in cases]
    return dict(B=c["B"], depth=_dev(c["depth"]), cam=ic.prepared(c["params"], c["models_frame"]), mask=_dev(c["mask"]), weights=_dev(c["weights"]),
                T=_dev(c["T"]), dist_tol=c["dist_tol"], cos_tol=c["cos_tol"], levels=levels)


def _chain(d, iters, *, filter=None, gate=math.inf, mask=None, weights=None, cos_tol=None, T=None):
    """track_camera_pyramid's definition spelled out"""
    from unidepth_amd import icp, normals, pyramid
    L = len(iters)
    res = pyramid.depth_pyramid(d["depth"], L, mask=mask, weights=weights, filter=filter, gate=gate)
    dl, wl = res if weights is not None else (res, [None] * L)
    cams = pyramid.pyramid_cameras(d["cam"], d["B"], L, "cuda")
    stats = []
    for l in reversed(range(L)):
        if iters[l] == 0:
            continue
        n = normals.normals_camera(dl[l], cams[l]) if cos_tol is not None else None
        T, st = icp.track_camera(dl[l], cams[l], *d["levels"][l], T, iters=iters[l], dist_tol=d["dist_tol"], cos_tol=cos_tol, normals=n, weights=wl[l])
        stats.append(st)
    return T, torch.cat(stats, dim=1)


def _same_track(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[1].dtype == torch.float64, what
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), f"{what}: T differs"
    assert torch.equal(got[1].view(torch.int64), want[1].view(torch.int64)), f"{what}: stats differ"


@pytest.mark.parametrize("frame_models,model_models", (((ic.PINHOLE,), (ic.PINHOLE,)), ((ic.PINHOLE, ic.SPHERICAL, ic.MEI), (ic.MEI, ic.PINHOLE, ic.OPENCV))))
def test_track_pyramid_is_the_explicit_chain(frame_models, model_models):
    """B = 1 and a mixed-model B = 3, frames of 37 x 53 against model maps of 48 x 64: T and stats bit-equal to the chain of depth_pyramid,
    pyramid_cameras and track_camera; plain, with an iters entry of 0, with the filter, gate, mask and weights, and with cos_tol"""
    from unidepth_amd import pyramid
    d = _track_case(frame_models, model_models, 3)
    f = _filter(2)
    for iters, kw in (((3, 2, 2), {}), ((2, 0, 3), {}), ((0, 2, 0), {}),
                      ((2, 2, 1), dict(filter=f, gate=0.3, mask=d["mask"], weights=d["weights"])),
                      ((2, 1, 2), dict(weights=d["weights"], cos_tol=d["cos_tol"]))):
        got = pyramid.track_camera_pyramid(d["depth"], d["cam"], d["levels"], d["T"], iters=iters, dist_tol=d["dist_tol"], **kw)
        assert got[0].shape == (d["B"], 3, 4) and got[1].shape == (d["B"], sum(iters), 4)
        _same_track(got, _chain(d, iters, T=d["T"], **kw), f"{frame_models} iters={iters} {sorted(kw)}")
    # the level cameras handed over ready-made, and no transform: the identity
    cams = pyramid.pyramid_cameras(d["cam"], d["B"], 3, "cuda")
    got = pyramid.track_camera_pyramid(d["depth"], cams, d["levels"], None, iters=(1, 1, 1), dist_tol=d["dist_tol"])
    _same_track(got, _chain(d, (1, 1, 1), T=None), "ready-made cameras")


def test_one_level_is_track_camera():
    from unidepth_amd import icp, pyramid
    d = _track_case((ic.PINHOLE, ic.EUCM), (ic.EUCM, ic.PINHOLE), 1)
    got = pyramid.track_camera_pyramid(d["depth"], d["cam"], d["levels"], d["T"], iters=(4,), dist_tol=d["dist_tol"], mask=d["mask"], weights=d["weights"])
    # the mask and the weights' liveness reach track_camera as depth 0: the same pixels are live, the same arithmetic follows
    want = icp.track_camera(d["depth"], d["cam"], *d["levels"][0], d["T"], iters=4, dist_tol=d["dist_tol"], mask=d["mask"], weights=d["weights"])
    _same_track(got, want, "L = 1")
    with pytest.raises(ValueError, match="point map"):
        pyramid.track_camera_pyramid(d["levels"][0][0], d["cam"], d["levels"], d["T"], iters=(4,), dist_tol=d["dist_tol"])


def test_track_pyramid_graph_replay():
    """captured once with prepared level cameras; replayed after the depth was rewritten in place: each replay equals a fresh call"""
    from unidepth_amd import pyramid
    d, e = _track_case((ic.PINHOLE, ic.EUCM, ic.MEI), (ic.MEI, ic.PINHOLE, ic.OPENCV), 3), _track_case((ic.PINHOLE, ic.EUCM, ic.MEI), (ic.MEI, ic.PINHOLE, ic.OPENCV), 3, seed=5)
    depth = d["depth"].clone()
    cams = pyramid.pyramid_cameras(d["cam"], d["B"], 3, "cuda")
    f = _filter(1)
    fn = lambda: pyramid.track_camera_pyramid(depth, cams, d["levels"], d["T"], iters=(2, 1, 2), dist_tol=d["dist_tol"], filter=f, weights=d["weights"])   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    for k in range(3):
        depth.copy_(e["depth"] if k % 2 == 0 else d["depth"])
        graph.replay()
        torch.cuda.synchronize()
        seen = (static[0].clone(), static[1].clone())
        _same_track(seen, fn(), f"replay {k}")


# ---- TsdfVolume.track_pyramid end to end -------------------------------------------------------------------------------------------------

VOLUME = dict(grid_shape=(48, 40, 40), voxel_size=0.078125, origin=(-1.5, -1.9, 0.0), trunc=0.25)      # tests/test_icp_gpu.py's fused corner
POSE_SIDE = ic.pose((0.0, 0.3, 0.0), (-0.5, 0.0, 0.2)) @ ic.POSE_A
SINGLE_LEVEL = (0.068, 0.0010)      # what TsdfVolume.track reaches on this scene from this start (profiles/scene_truth.txt): degrees, translation


def test_volume_track_pyramid_end_to_end():
    """the fused corner of tests/test_icp_gpu.py's test_volume_track_end_to_end -- the views A and one sideways (96 x 128, f 80) fused
    into 40 x 40 x 48 voxels of 5/64, rendered at A at 48 x 64, 24 x 32 and 12 x 16, the frame from B, the start A: 3.08 degrees /
    0.0707.  With r = 0, gate = inf and iters (10, 5, 4) the pose must end within 1.5 times what the single-level track reaches there,
    0.068 degrees / 0.0010: the last level is the raw frame at full resolution, so the fixed point is the same.  (The corner is the
    analytic scene of tests/icp_common.py; its pose errors are taken against the analytic POSE_B.)  Printed and not asserted (the basin
    is bounded by dist_tol more than by the pixel size, profiles/pyramid_track.txt): the same from twice the start, single-level and
    pyramid, and with the r = 2 filter.

    Measured on the MI355X (profiles/pyramid_track.txt), degrees / translation: from the start the single level (iters 10) ends at
    0.0679 / 0.000997 and the pyramid at 0.0679 / 0.000998; from twice the start (6.17 / 0.1414) 0.0774 / 0.000900 and 0.0765 / 0.000885;
    with the r = 2 filter 0.1019 / 0.003752 and 0.0993 / 0.003804 (the filter rounds the creases of the corner)."""
    from unidepth_amd import tsdf
    Hs, Ws, fs = 96, 128, 80.0
    views = np.stack([ic.corner_view(P, Hs, Ws, fs)[0] for P in (ic.POSE_A, POSE_SIDE)]).astype(F)
    big = ic.prepared(ic.pinhole_row(Hs, Ws, fs)[None], (ic.PINHOLE,))
    vol = tsdf.tsdf_integrate(None, _dev(views[None]), [big, big], _dev(np.stack([ic.POSE_A, POSE_SIDE]).astype(F)), **VOLUME)
    H, W, f = 48, 64, 40.0
    cam = ic.prepared(ic.pinhole_row(H, W, f)[None], (ic.PINHOLE,))
    frame = _dev(ic.corner_view(ic.POSE_B, H, W, f)[0].astype(F)[None, None])
    D = ic.POSE_B @ np.linalg.inv(ic.POSE_A)
    starts = {"start": ic.POSE_A, "twice the start": np.linalg.inv(D) @ ic.POSE_A}
    kw = dict(near=0.3, far=5.0, dist_tol=0.2)
    lines = {}
    for name, P in starts.items():
        prior = _dev(P.astype(F))
        runs = {"single level, iters 10": lambda: vol.track(frame, cam, (H, W), prior, iters=10, **kw),
                "pyramid (10, 5, 4)": lambda: vol.track_pyramid(frame, cam, (H, W), prior, levels=3, iters=(10, 5, 4), **kw),
                "pyramid (10, 5, 4), r = 2": lambda: vol.track_pyramid(frame, cam, (H, W), prior, levels=3, iters=(10, 5, 4), gate=0.1,
                                                                       filter=_filter(2, 0.05), **kw)}
        for run, fn in runs.items():
            T, stats = fn()
            lines[name, run] = ic.pose_errors(T[0].cpu().numpy(), ic.POSE_B)
            print(f"pyramid_track: {name} {ic.pose_errors(P, ic.POSE_B)[0]:.3f} deg / {ic.pose_errors(P, ic.POSE_B)[1]:.4f}, {run}: "
                  f"{lines[name, run][0]:.4f} deg / {lines[name, run][1]:.6f}, steps ok {int(stats[0, :, 3].sum())} of {stats.shape[1]}, "
                  f"matched at the last step {int(stats[0, -1, 2])}")
    T, stats = vol.track_pyramid(frame, cam, (H, W), _dev(ic.POSE_A.astype(F)), levels=3, iters=(10, 5, 4), **kw)
    assert T.shape == (1, 3, 4) and T.dtype == torch.float32 and stats.shape == (1, 19, 4) and stats.dtype == torch.float64
    start, reached = ic.pose_errors(ic.POSE_A, ic.POSE_B), lines["start", "pyramid (10, 5, 4)"]
    assert abs(start[0] - 3.08) < 0.01 and abs(start[1] - 0.0707) < 1e-4
    bar = tuple(1.5 * m for m in SINGLE_LEVEL)
    assert reached[0] <= bar[0] and reached[1] <= bar[1], (reached, bar)
    # an iters entry of 0 skips its level's render as well; (n, 0, 0) is the single-level track
    T1, s1 = vol.track_pyramid(frame, cam, (H, W), _dev(ic.POSE_A.astype(F)), levels=3, iters=(8, 0, 0), **kw)
    T0, s0 = vol.track(frame, cam, (H, W), _dev(ic.POSE_A.astype(F)), iters=8, **kw)
    _same_track((T1, s1), (T0, s0), "iters (8, 0, 0) against track")
