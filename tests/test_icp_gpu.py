"""GPU parity of icp_linearize / icp_solve / track_camera (unidepth_amd/icp.py -> ud_icp_linearize, ud_icp_update, csrc/icp.hip) against
the composition of the merged calls -- gt_points, project_camera, remap(mode="nearest") and torch element-wise arithmetic -- bit for bit
in matched, residual and rows at every pixel: both sides run the same functions of camera_models.h and remap_taps.h under
-ffp-contract=off.  The fp64 sums are compared with torch.sum's within the bound of two summation orders, the count exactly; the solve
with the numpy restatement of tests/icp_common.py, bit for bit, fed the device's own system; the loop with the composition's loop and
with both known answers.  The scenes are those of tests/icp_common.py, whose conditions tests/test_icp_cpu.py asserts on the host
program; the raw C-ABI call writes into guarded allocations (tests/layout_guard.py), the uint8 outputs at odd byte offsets."""
import numpy as np
import pytest
import torch

import icp_common as ic
import layout_guard as lg

CORNER_MEASURED, SMOOTH_FLOOR = ic.CORNER_MEASURED, ic.SMOOTH_FLOOR

pytestmark = pytest.mark.gpu
_SENTINEL_BYTES = (0xAD, 0xDB, 0xBA, 0x7F)                     # lg.SENTINEL[torch.float32], little endian
NAMES = ("system", "matched", "residual", "rows")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _device_case(c):
    d = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    d["cam"] = ic.prepared(c["params"], c["models_frame"])
    d["mcam"] = ic.prepared(c["params_model"], c["models_model"])
    return d


def _options(d, mask, weights, normals):
    kw = {}
    if mask:
        kw["mask"] = d["mask"]
    if weights:
        kw["weights"] = d["weights"]
    if normals:
        kw["normals"], kw["cos_tol"] = d["normals"], d["cos_tol"]
    return kw


def _args(d, frame=None, camera=None):
    return (d["depth"] if frame is None else frame, d["cam"] if camera is None else camera, d["mp"], d["mn"], d["mv"], d["mcam"], d["T"])


def _assert_system(S, want, matched, residual, rows, weights, what):
    """the device's sums against torch.sum's of the same terms: |dS| <= 2 n 2^-53 sum |t| per slot, the count exact, the tail zero"""
    S, want = S.cpu().numpy(), want.cpu().numpy()
    m, r, g = matched.cpu().numpy(), residual.cpu().numpy(), rows.cpu().numpy()
    for b in range(S.shape[0]):
        w = np.ones(m[b, 0].shape, np.float32) if weights is None else weights[b].cpu().numpy().reshape(m[b, 0].shape)
        bound = ic.system_bound(ic.terms(m[b, 0], r[b, 0], g[b], w))
        assert (np.abs(S[b] - want[b]) <= bound).all(), (what, b, np.abs(S[b] - want[b]).max(), bound.max())
        assert S[b, 29] == want[b, 29] == m[b].sum() and S[b, 30] == 0 and S[b, 31] == 0, (what, b)


def _both(d, what, frame=None, camera=None, **kw):
    """the fused call and the composition on the same arguments: the per-pixel outputs bit for bit, the sums within the bound -> the fused
    call's results"""
    from unidepth_amd import icp
    got = icp.icp_linearize(*_args(d, frame, camera), dist_tol=d["dist_tol"], return_rows=True, **kw)
    want = icp.icp_linearize_composition(*_args(d, frame, camera), dist_tol=d["dist_tol"], return_rows=True, **kw)
    B, H, W = d["B"], d["H"], d["W"]
    assert got[0].shape == (B, 32) and got[0].dtype == torch.float64 and got[1].shape == (B, 1, H, W) and got[1].dtype == torch.bool
    assert got[2].shape == (B, 1, H, W) and got[3].shape == (B, 6, H, W)
    ic.host_program.assert_same(got[1:], want[1:], NAMES[1:], what)
    off = ~got[1]
    assert not bool(ic.bits(got[2])[off].any()) and not bool(ic.bits(got[3])[off.expand(B, 6, H, W)].any()), what
    _assert_system(got[0], want[0], got[1], got[2], got[3], kw.get("weights"), what)
    alone = icp.icp_linearize(*_args(d, frame, camera), dist_tol=d["dist_tol"], **kw)
    assert torch.equal(alone.view(torch.int64), got[0].view(torch.int64)), f"{what}: two calls gave different sums"
    return dict(zip(NAMES, got))


@pytest.mark.parametrize("frame_model", ic.CLOSED, ids=[ic.NAMES[m] for m in ic.CLOSED])
def test_matrix_against_the_composition(frame_model):
    """a frame of one closed-form model against a batch of all six model cameras, 29x41 against 37x53; shared and per-image T; mask,
    weights and normals + cos_tol each on and off"""
    for per_image in (False, True):
        d = _device_case(ic.mixed_case((frame_model,) * 6, ic.MODELS, per_image=per_image))
        for mask, weights, normals in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            r = _both(d, f"{ic.NAMES[frame_model]} per_image={per_image} {mask}{weights}{normals}", **_options(d, mask, weights, normals))
            share = r["matched"].float().mean(dim=(1, 2, 3))
            assert bool((share > 0.05).all()) and bool((share < 0.95).all()), share


def test_mixed_batch_and_points_form():
    """B = 3 mixing frame and model cameras; the points form; and an OPENCV and a Fisheye624 frame with a depth, which the wrapper routes
    through gt_points into the points form (the entry point refuses them in the depth form)"""
    from unidepth_amd import gtpoints, icp
    d = _device_case(ic.mixed_case((ic.PINHOLE, ic.SPHERICAL, ic.MEI), (ic.EUCM, ic.FISHEYE624, ic.PINHOLE)))
    base = _both(d, "mixed B=3", **_options(d, 1, 1, 1))
    pts = gtpoints.gt_points(d["depth"], d["cam"])
    r = _both(d, "points form", frame=pts, **_options(d, 1, 1, 1))
    ic.host_program.assert_same(tuple(r[k] for k in NAMES[1:]), tuple(base[k] for k in NAMES[1:]), NAMES[1:], "points form vs depth form")
    assert torch.equal(r["system"].view(torch.int64), base["system"].view(torch.int64))
    c = ic.mixed_case((ic.OPENCV, ic.FISHEYE624, ic.OPENCV), (ic.PINHOLE, ic.MEI, ic.OPENCV))
    d = _device_case(c)
    r = _both(d, "iterative frames", **_options(d, 1, 0, 1))
    assert 0.05 < float(r["matched"].float().mean()) < 0.95
    with pytest.raises(RuntimeError, match="iterative frame model"):
        _raw(d, want=())


EDGE_WIDTHS = (63, 64, 65, 255, 256, 257, ic.SPAN - 1, ic.SPAN, ic.SPAN + 1)


@pytest.mark.parametrize("W", EDGE_WIDTHS)
def test_edge_frames(W):
    """1 x N frames around the wave, the workgroup and the grid-stride span of 65,536 pixels (256 workgroups of 256 threads per image)"""
    d = _device_case(ic.mixed_case((ic.PINHOLE, ic.EUCM), (ic.MEI, ic.PINHOLE), H=1, W=W, Hm=5, Wm=61))
    r = _both(d, f"1x{W}", **_options(d, 1, 1, 0))
    assert bool(r["matched"].any()) and not bool(r["matched"].all())


def test_workgroups_per_image_change_no_row():
    """UdIcp.blocks (icp._LAUNCH_OPTIONS, the benchmark's sweep): 1, 3, 512 and 1024 workgroups per image on a frame of 4 * 65,536 + 1
    pixels, where each of them differs from the default 256 -- the same rows bit for bit, the sums within the bound and reproducible,
    the partials of more than one chunk of 128 summed by the second launch"""
    from unidepth_amd import icp
    d = _device_case(ic.mixed_case((ic.PINHOLE, ic.EUCM), (ic.MEI, ic.PINHOLE), H=1, W=4 * ic.SPAN + 1, Hm=5, Wm=61))
    base = _both(d, "default", **_options(d, 1, 1, 0))
    try:
        for blocks in (1, 3, 512, 1024):
            icp._LAUNCH_OPTIONS["blocks"] = blocks
            r = _both(d, f"blocks={blocks}", **_options(d, 1, 1, 0))
            ic.host_program.assert_same(tuple(r[k] for k in NAMES[1:]), tuple(base[k] for k in NAMES[1:]), NAMES[1:], f"blocks={blocks}")
            assert torch.equal(r["system"][:, 29], base["system"][:, 29])
    finally:
        icp._LAUNCH_OPTIONS["blocks"] = 0


def test_edge_model_maps_and_batch_of_256():
    from unidepth_amd import icp
    hits = 0
    for Hm, Wm in ((1, 1), (2, 3)):
        d = _device_case(ic.mixed_case((ic.PINHOLE, ic.EUCM, ic.MEI), (ic.PINHOLE, ic.OPENCV, ic.SPHERICAL), H=2, W=3, Hm=Hm, Wm=Wm))
        hits += int(_both(d, f"model {Hm}x{Wm}", **_options(d, 1, 1, 0))["matched"].sum())
    models = tuple(ic.CLOSED[b % 4] for b in range(256))
    d = _device_case(ic.mixed_case(models, tuple(ic.MODELS[b % 6] for b in range(256)), H=1, W=1, Hm=1, Wm=1))
    r = _both(d, "B=256 of 1x1")
    hits += int(r["matched"].sum())
    assert hits > 0
    T, x, status = icp.icp_solve(r["system"], d["T"])
    assert T.shape == (256, 3, 4) and not bool(status.any()) and torch.equal(T, d["T"]) and not bool(x.any())       # one pixel: singular


def test_special_values():
    c = ic.special_case()
    d = _device_case(c)
    r = _both(d, "special", **_options(d, 1, 1, 1))
    m = r["matched"].cpu().numpy()[:, 0]
    assert not m[0].reshape(-1)[:6].any() and not m[0].reshape(-1)[8:13].any()
    assert not m[2].any() and not m[3].any() and not m[4].any() and m[0].any() and m[1].any()
    assert bool(torch.isfinite(r["system"]).all()) and not bool(r["system"][2:, :30].any())
    raw = _raw(d, **_options(d, 1, 1, 1))
    ic.host_program.assert_same(tuple(raw[k] for k in NAMES[1:]), tuple(r[k] for k in NAMES[1:]), NAMES[1:], "special raw")


# ---- the C-ABI on guarded allocations ------------------------------------------------------------------------------------------------

class _Out:
    """`n` elements of `dtype`, `offset` elements into a sentinel-filled allocation: the guard rows above and below are checked by
    layout_guard, the bytes of the view's own words before and after the elements here"""

    def __init__(self, n, dtype, offset=0):
        esz = torch.empty(0, dtype=dtype).element_size()
        self.words = max(1, -(-(n + offset) * esz // 4))
        self.g = lg.guarded(self.words, 1, 1, torch.float32)
        self.bytes = self.g.view.reshape(-1).view(torch.uint8)
        self.lo, self.hi = offset * esz, (offset + n) * esz
        self.t = self.bytes[self.lo:self.hi].view(dtype)

    def check(self, name, written=True):
        self.g.check_guards(name)
        want = torch.tensor(_SENTINEL_BYTES, dtype=torch.uint8, device="cuda").repeat(self.words)
        keep = torch.ones_like(want, dtype=torch.bool)
        if written:
            keep[self.lo:self.hi] = False
        assert torch.equal(self.bytes[keep], want[keep]), f"{name}: bytes beside the output were rewritten" if written else f"{name}: an absent output was written"


def _raw(d, *, want=("matched", "residual", "rows"), solve=False, mask=None, weights=None, normals=None, cos_tol=None, work_bytes=None, T=None):
    """ud_icp_linearize through the C-ABI on device tensors, every output inside a guarded allocation (absent ones too: they must stay
    untouched), twice, the workspace filled with NaN before the second call -> dict of the outputs asked for, in the wrapper's shapes"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    B, H, W = d["B"], d["H"], d["W"]
    n = B * H * W
    nbytes = int(_lib.lib.ud_icp_workspace_bytes(B, H, W))
    bufs = dict(system=_Out(B * 32, torch.float64, 2), matched=_Out(n, torch.uint8, 3), residual=_Out(n, torch.float32, 1), rows=_Out(6 * n, torch.float32, 3),
                x=_Out(B * 6, torch.float64), status=_Out(B, torch.uint8, 1), stats=_Out(B * 4, torch.float64, 2), work=_Out(nbytes // 8, torch.float64, 2))
    has = {k: k in ("system", "work") or k in want or (solve and k in ("x", "status", "stats")) for k in bufs}
    T0 = (d["T"] if T is None else T).reshape(-1, 3, 4).contiguous()
    if solve:
        T0 = T0.expand(B, 3, 4).contiguous()
    runs = []
    for k in range(2):
        Tk = T0.clone()
        desc = mk(_lib.UdIcp, depth=d["depth"].contiguous(), params=d["cam"].params, mask=mask, weights=weights, normals=normals, model_points=d["mp"],
                  model_normals=d["mn"], model_valid=d["mv"], params_model=d["mcam"].params, T=Tk, work_bytes=nbytes if work_bytes is None else work_bytes,
                  B=B, H=H, W=W, Hm=d["Hm"], Wm=d["Wm"], nT=Tk.shape[0], solve=int(solve), min_count=6, has_cos=int(cos_tol is not None),
                  dist_tol_bits=ic.f32_bits(d["dist_tol"]), cos_tol_bits=ic.f32_bits(cos_tol or 0.0), stats_stride=4,
                  **{name: (b.t.data_ptr() if has[name] else None) for name, b in bufs.items()})
        for b in range(B):
            desc.model_frame[b], desc.model_model[b] = d["cam"].models[b], d["mcam"].models[b]
        if k == 1:
            bufs["work"].t.fill_(float("nan"))
        check(_lib.lib.ud_icp_linearize(desc, cur_stream()), "ud_icp_linearize")
        torch.cuda.synchronize()
        runs.append({name: b.t.clone() for name, b in bufs.items() if has[name] and name != "work"})
        runs[-1]["T"] = Tk
    for name, b in bufs.items():
        b.check(name, has[name])
    for name in runs[0]:
        assert torch.equal(ic.bits(runs[0][name].view(torch.int64) if runs[0][name].dtype == torch.float64 else runs[0][name]),
                           ic.bits(runs[1][name].view(torch.int64) if runs[1][name].dtype == torch.float64 else runs[1][name])), \
            f"two calls (the second on a workspace of NaN) gave different bits in {name}"
    r = runs[0]
    shape = dict(system=(B, 32), matched=(B, 1, H, W), residual=(B, 1, H, W), rows=(B, 6, H, W), x=(B, 6), status=(B,), stats=(B, 4), T=(-1, 3, 4))
    return {name: (t.view(shape[name]).bool() if name == "matched" else t.view(shape[name])) for name, t in r.items()}


def test_guarded_c_abi():
    """the entry point itself on guarded allocations at odd byte offsets: absent optional outputs stay untouched, guard bytes stay intact,
    two calls give the same bits (the second on a workspace filled with NaN), the bits are the wrapper's, and a workspace that is too
    small is refused"""
    from unidepth_amd import icp
    for c in (ic.mixed_case((ic.PINHOLE, ic.EUCM, ic.SPHERICAL, ic.MEI), (ic.MEI, ic.OPENCV, ic.PINHOLE, ic.FISHEYE624)),
              ic.mixed_case((ic.PINHOLE, ic.MEI), (ic.EUCM, ic.PINHOLE), H=1, W=257, Hm=3, Wm=41)):
        d = _device_case(c)
        kw = _options(d, 1, 1, 1)
        full = _raw(d, **kw)
        want = icp.icp_linearize(*_args(d), dist_tol=d["dist_tol"], return_rows=True, **kw)
        ic.host_program.assert_same(tuple(full[k] for k in NAMES[1:]), want[1:], NAMES[1:], "raw")
        assert torch.equal(full["system"].view(torch.int64), want[0].view(torch.int64))
        for keep in ((), ("matched",), ("residual",), ("rows",)):
            part = _raw(d, want=keep, **kw)
            assert set(part) == {"system", "T", *keep}
            assert torch.equal(part["system"].view(torch.int64), full["system"].view(torch.int64)) and torch.equal(part["T"], d["T"])
        plain = _raw(d, want=("matched",))
        assert not torch.equal(plain["matched"], full["matched"])
        # with the solve: x, status, the stats row and T in place, as icp_solve gives them
        s = _raw(d, want=(), solve=True, **kw)
        Tn, x, status = icp.icp_solve(full["system"], d["T"])
        assert torch.equal(ic.bits(s["T"]), ic.bits(Tn)) and torch.equal(s["x"].view(torch.int64), x.view(torch.int64)) and torch.equal(s["status"].bool(), status)
        assert torch.equal(s["stats"][:, :3].view(torch.int64), full["system"][:, 27:30].contiguous().view(torch.int64)) and torch.equal(s["stats"][:, 3] != 0, status)
        if d["H"] > 1:                                   # (a frame of one row constrains too little: every status is 0 there)
            assert bool(status.any()) and not bool(status.all()) and not torch.equal(Tn, d["T"])
        with pytest.raises(RuntimeError, match="workspace"):
            _raw(d, work_bytes=8)


# ---- the solve and the loop ----------------------------------------------------------------------------------------------------------

def _scene_args(s):
    cam, mcam = ic.prepared(s["row"][None], (ic.PINHOLE,)), ic.prepared(s["row_model"][None], (ic.PINHOLE,))
    return (_dev(s["depth"][None, None]), cam, _dev(s["mp"][None]), _dev(s["mn"][None]), _dev(s["mv"][None, None]), mcam, _dev(s["T0"][None]))


SCENES = [("corner", k) for k in ic.CORNER_SIZES] + [("smooth", k) for k in ic.SMOOTH_SIZES]


def test_solve_equals_the_restatement_on_the_device_sums():
    """icp_solve, fed the device's own systems of all seven scenes, against the numpy fp64 restatement: x, status and T_new bit for bit
    (fp64 + - * / correctly rounded on the device, no contraction); with damping, with count below min_count, with a NaN entry, and on
    the singular system of a single pixel"""
    from unidepth_amd import icp
    S, T = [], []
    for kind, key in SCENES:
        s = ic.corner(key) if kind == "corner" else ic.smooth(key)
        a = _scene_args(s)
        S.append(icp.icp_linearize(*a, dist_tol=s["dist_tol"]))
        T.append(a[6])
    S, T = torch.cat(S), torch.cat(T)
    Sn = S.clone()
    Sn[2, 3], Sn[5, 22] = float("nan"), float("nan")
    T0 = T.clone()
    for Sk, kw in ((S, {}), (S, dict(damping=5.0)), (S, dict(min_count=10 ** 6)), (Sn, {})):
        Tn, x, status = icp.icp_solve(Sk, T, **kw)
        assert Tn.dtype == torch.float32 and x.dtype == torch.float64 and status.dtype == torch.bool and torch.equal(T, T0)
        for b in range(len(SCENES)):
            wT, wx, ws = ic.solve(Sk[b].cpu().numpy(), T[b].cpu().numpy(), **kw)
            assert bool(status[b]) == bool(ws) and ic.same_bits(x[b].cpu().numpy(), wx) and ic.same_bits(Tn[b].cpu().numpy(), wT), (kw, b, x[b], wx)
    # the torch restatement the composition's loop uses is the same function
    Tr, xr, sr = icp._solve_restated(S, T, 0.0, 6)
    Tn, x, status = icp.icp_solve(S, T)
    assert torch.equal(ic.bits(Tr), ic.bits(Tn)) and torch.equal(xr.view(torch.int64), x.view(torch.int64)) and torch.equal(sr, status)


@pytest.mark.parametrize("kind,key", SCENES, ids=[f"{a}_{b}" for a, b in SCENES])
def test_track_camera_against_the_composition(kind, key):
    """the fused loop and the composition's loop from the same start: the same matched counts and statuses at every iteration, T within
    4 fp32 ulp per entry at the end (the iterates can differ only through the order of the fp64 sums), and the known answer: the corner
    after 8 iterations within 0.25 degrees and 0.01, the smooth surface after 6 within 8 times the floor measured with the restatement"""
    from unidepth_amd import icp
    s = ic.corner(key) if kind == "corner" else ic.smooth(key)
    iters = 8 if kind == "corner" else 6
    a = _scene_args(s)
    T, stats = icp.track_camera(*a, iters=iters, dist_tol=s["dist_tol"])
    Tc, stats_c = icp.track_camera_composition(*a, iters=iters, dist_tol=s["dist_tol"])
    assert T.shape == (1, 3, 4) and stats.shape == (1, iters, 4) and stats.dtype == torch.float64
    assert torch.equal(stats[..., 2:], stats_c[..., 2:]), (stats[0, :, 2], stats_c[0, :, 2])
    Th, Tch = T[0].cpu().numpy(), Tc[0].cpu().numpy()
    ulps = np.abs(Th.astype(np.float64) - Tch) / np.spacing(np.abs(Tch)).astype(np.float64)
    rot, tr = ic.pose_errors(Th, s["truth"])
    print(f"{kind} {key}: T differs from the composition's by at most {ulps.max()} ulp; errors {rot} degrees, {tr}")
    assert ulps.max() <= 4
    n_live = float((s["depth"] > 0).sum())
    share = stats[0, :, 2].cpu().numpy() / n_live
    assert (share >= 0.5).all() and (share <= 0.95).all() and bool((stats[0, :, 3] == 1).all()), share
    if kind == "corner":
        assert rot <= ic.CORNER_BARS[0] and tr <= ic.CORNER_BARS[1], (rot, tr)
        assert rot <= 1.01 * CORNER_MEASURED[key][0] and tr <= 1.01 * CORNER_MEASURED[key][1], (rot, tr)
    else:
        assert rot <= 8 * SMOOTH_FLOOR[0] and tr <= 8 * SMOOTH_FLOOR[1], (rot, tr)
    # transform=None is the identity, the corner's start
    if kind == "corner":
        Tn, _ = icp.track_camera(*a[:6], None, iters=iters, dist_tol=s["dist_tol"])
        assert torch.equal(Tn, T)
    # a failed step leaves T as it was and the later steps still run
    Tf, sf = icp.track_camera(*a, iters=3, dist_tol=s["dist_tol"], min_count=10 ** 6)
    assert torch.equal(Tf, a[6]) and not bool(sf[..., 3].any()) and bool((sf[..., 2] == sf[0, 0, 2]).all()) and bool((sf[..., 2] > 0).all())


# ---- TsdfVolume.track ----------------------------------------------------------------------------------------------------------------

VOLUME = dict(grid_shape=(48, 40, 40), voxel_size=0.078125, origin=(-1.5, -1.9, 0.0), trunc=0.25)
# x in -1.5 .. 1.625, y in -1.9 .. 1.225, z in 0 .. 3.75: the planes x = -1.2, y = 1.0 and z = 3.0 lie 3.8, 2.9 and 9.6 voxels inside
POSE_SIDE = ic.pose((0.0, 0.3, 0.0), (-0.5, 0.0, 0.2)) @ ic.POSE_A
# what TsdfVolume.track reaches in the test below (rotation error in degrees, translation error against POSE_B), measured on the MI355X
# and rounded up in the last digit: the floor of the discretised surface (profiles/scene_truth.txt)
END_TO_END_MEASURED = (0.0679, 0.000998)


def test_volume_track_end_to_end():
    """the corner fused by tsdf_integrate from the views A and one sideways (96x128, f 80) into a 40x40x48 grid of 5/64 voxels at
    (-1.5, -1.9, 0), trunc 0.25; rendered at A (48x64, f 40), the frame from B: the volume->camera transform returned is closer to B than
    the start A in rotation and in translation (the start: 3.08 degrees, 0.0707), and integrating the frame with it changes the volume.
    The errors reached are printed and held under a bar measured against the analytic truth (tests/test_scene_truth_gpu.py measures
    the whole chain the same way)."""
    from unidepth_amd import tsdf
    Hs, Ws, fs = 96, 128, 80.0
    views = np.stack([ic.corner_view(P, Hs, Ws, fs)[0] for P in (ic.POSE_A, POSE_SIDE)]).astype(np.float32)
    big = ic.prepared(ic.pinhole_row(Hs, Ws, fs)[None], (ic.PINHOLE,))
    Tv = _dev(np.stack([ic.POSE_A, POSE_SIDE]).astype(np.float32))
    vol = tsdf.tsdf_integrate(None, _dev(views[None]), [big, big], Tv, **VOLUME)
    H, W, f = 48, 64, 40.0
    cam = ic.prepared(ic.pinhole_row(H, W, f)[None], (ic.PINHOLE,))
    frame = _dev(ic.corner_view(ic.POSE_B, H, W, f)[0].astype(np.float32)[None, None])
    prior = _dev(ic.POSE_A.astype(np.float32))
    T, stats = vol.track(frame, cam, (H, W), prior, near=0.3, far=5.0, iters=8, dist_tol=0.2)
    assert T.shape == (1, 3, 4) and T.dtype == torch.float32 and stats.shape == (1, 8, 4) and bool((stats[..., 3] == 1).all())
    start, reached = ic.pose_errors(ic.POSE_A, ic.POSE_B), ic.pose_errors(T[0].cpu().numpy(), ic.POSE_B)
    print(f"TsdfVolume.track: start {start}, reached {reached}, matched {stats[0, :, 2].tolist()}")
    assert reached[0] < start[0] and reached[1] < start[1], (start, reached)
    # the bar on the reached pose: 1.5 times what the correct chain measures against the analytic truth POSE_B (END_TO_END_MEASURED);
    # the same result composed the wrong way round, E . prior for invert_rigid(E) . prior, must lie at least twice the bar away
    bar = tuple(1.5 * m for m in END_TO_END_MEASURED)
    assert reached[0] <= bar[0] and reached[1] <= bar[1], (reached, bar)
    got, A = np.eye(4), np.eye(4)
    got[:3], A[:3] = T[0].cpu().numpy(), ic.POSE_A[:3]
    E = A @ np.linalg.inv(got)                                       # got = E^-1 prior
    wrong = ic.pose_errors(E @ A, ic.POSE_B)
    print(f"TsdfVolume.track: composed the wrong way round {wrong}, bar {bar}")
    assert wrong[0] >= 2 * bar[0] and wrong[1] >= 2 * bar[1], (wrong, bar)
    before = vol.tsdf.clone()
    tsdf.tsdf_integrate(vol, frame, [cam], T[None], trunc=VOLUME["trunc"])
    assert not torch.equal(before, vol.tsdf)


# ---- graph replay --------------------------------------------------------------------------------------------------------------------

def test_graph_replay_after_inputs_were_rewritten():
    """track_camera captured once with PreparedCameras; replayed after the depth, the model maps, T and camera rows were rewritten in
    place: each replay equals a fresh call"""
    from unidepth_amd import gtpoints, icp
    c, e = ic.mixed_case((ic.PINHOLE, ic.EUCM, ic.MEI), (ic.MEI, ic.PINHOLE, ic.OPENCV)), ic.mixed_case((ic.PINHOLE, ic.EUCM, ic.MEI), (ic.MEI, ic.PINHOLE, ic.OPENCV), seed=5)
    d, e = _device_case(c), _device_case(e)
    depth, mp, mn, mv, T = d["depth"].clone(), d["mp"].clone(), d["mn"].clone(), d["mv"].clone(), d["T"].clone()
    cam = gtpoints.PreparedCamera(d["cam"].params.clone(), d["cam"].models)
    mcam = gtpoints.PreparedCamera(d["mcam"].params.clone(), d["mcam"].models)
    kw = dict(iters=4, dist_tol=d["dist_tol"], mask=d["mask"], weights=d["weights"])
    fn = lambda: icp.track_camera(depth, cam, mp, mn, mv, mcam, T, **kw)             # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    seen = []
    for k in range(3):
        depth.copy_(e["depth"] if k % 2 == 0 else d["depth"])
        mp.copy_(e["mp"] if k % 2 == 0 else d["mp"])
        mv.copy_(e["mv"] if k % 2 == 0 else d["mv"])
        T[1].copy_(e["T"][1] if k % 2 == 0 else d["T"][1])
        cam.params[2, :2].mul_(1.02 if k % 2 == 0 else 0.97)
        mcam.params[0, 2:4].add_(0.25 if k % 2 == 0 else -0.125)
        graph.replay()
        torch.cuda.synchronize()
        fresh = fn()
        assert torch.equal(ic.bits(static[0]), ic.bits(fresh[0])) and torch.equal(static[1].view(torch.int64), fresh[1].view(torch.int64)), f"replay {k}"
        assert bool((static[1][..., 2] > 0).all())
        seen.append(static[0].clone())
    assert not torch.equal(seen[0], seen[1])
