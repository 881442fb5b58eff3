"""GPU parity of tsdf_render (unidepth_amd/tsdf.py -> ud_tsdf_render, csrc/tsdf_render.hip) against the numpy fp32 restatement of the full
scan in tests/tsdf_render_common.py, run on the rays form, bit for bit in depth, valid, points, normals and colour at every pixel: the
fused kernel is never its own oracle.  The camera form is compared with unproject_camera(normalize=True) + the rays form, and
tsdf_render_composition, the torch loop over the samples, is a second oracle on two small scenes.  The volumes come from tsdf_integrate on
the scenes of tests/tsdf_common.py, whose shares tests/test_tsdf_render_cpu.py asserts on the host program; the raw C-ABI calls write into
guarded allocations (tests/layout_guard.py) at odd offsets."""
import functools

import numpy as np
import pytest
import torch

import tsdf_common as tc
import tsdf_render_common as rc
from test_tsdf_gpu import _Out, _dev

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("depth", "valid", "points", "normals", "color")
ALL = dict(return_points=True, return_normals=True, return_color=True)


@functools.lru_cache(maxsize=None)
def _volumes(second=False, per_origin=False, B=2, colour=True):
    """tsdf_integrate on tsdf_common's scene -> (the TsdfVolume, its numpy form for the restatement)"""
    from unidepth_amd import tsdf
    s = tc.scene(tc.mixed_models(B=B), B=B, per_origin=per_origin, **(tc.SECOND if second else tc.BASE))
    cams = [tc.prepared(s["params"][v], s["models"][v]) for v in range(s["V"])]
    vol = tsdf.tsdf_integrate(None, _dev(s["depths"]), cams, _dev(s["T"]), grid_shape=s["grid"], origin=_dev(s["origin"]), voxel_size=s["voxel"],
                              trunc=s["trunc"], src_weights=_dev(s["src_weights"]), images=_dev(s["images"]) if colour else None)
    return vol, _numpy(vol)


def _numpy(vol):
    B, Nz, Ny, Nx = vol.tsdf.shape
    return dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=None if vol.color is None else vol.color.cpu().numpy(),
                origin=vol.origin.cpu().numpy(), voxel=vol.voxel_size, grid=(Nz, Ny, Nx), B=B)


def _upload(v):
    from unidepth_amd import tsdf
    return tsdf.TsdfVolume(_dev(v["tsdf"]), _dev(v["weight"]), None if v["color"] is None else _dev(v["color"]), _dev(v["origin"]), v["voxel"])


def _as_dict(res, points=True, normals=True, color=None):
    """tsdf_render's tuple as the restatement's dict (numpy)"""
    res = list(res)
    d = dict(depth=res.pop(0).cpu().numpy(), valid=res.pop(0).cpu().numpy(), points=None, normals=None, color_f32=None, color_u8=None)
    if points:
        d["points"] = res.pop(0).cpu().numpy()
    if normals:
        d["normals"] = res.pop(0).cpu().numpy()
    if color is not None:
        d["color_f32" if color == torch.float32 else "color_u8"] = res.pop(0).cpu().numpy()
    assert not res
    return d


def _check(vol, vnp, models, size=rc.SIZE, T_vc=None, rays=None, what="", camera_form=True, **kw):
    """tsdf_render in the rays form against the restatement on the same directions; the camera form (closed-form models) and the fp32
    colours against the rays form -> the restatement's result"""
    from unidepth_amd import tsdf, unproject
    cam = tc.prepared(rc.params_for(models, size), models)
    T = None if T_vc is None else _dev(T_vc)
    dirs = _dev(rays) if rays is not None else unproject.unproject_camera(None, cam, normalize=True, image_shape=size)
    want = rc.restate(vnp, models, dirs.cpu().numpy(), None if T_vc is None else rc.invert(T_vc), **kw)
    col = vnp["color"] is not None
    opts = dict(return_points=True, return_normals=True, return_color=col, **{**dict(near=rc.NEAR, far=rc.FAR), **kw})
    got = _as_dict(tsdf.tsdf_render(vol, cam, size, T, rays=dirs, **opts), color=torch.uint8 if col else None)
    names = ("depth", "valid", "points", "normals") + (("color_u8",) if col else ())
    rc.assert_same(got, want, what + " rays form", names)
    if col:
        f32 = _as_dict(tsdf.tsdf_render(vol, cam, size, T, rays=dirs, color_dtype=torch.float32, **opts), color=torch.float32)
        rc.assert_same(f32, want, what + " fp32 colours", names[:4] + ("color_f32",))
    if rays is None and camera_form:
        fused = _as_dict(tsdf.tsdf_render(vol, cam, size, T, **opts), color=torch.uint8 if col else None)
        rc.assert_same(fused, got, what + " camera form", names)
    return want


# ---- fused against the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", rc.CLOSED)
def test_camera_form_equals_rays_form_equals_restatement(model):
    """each closed-form camera: fused == unproject_camera(normalize=True) + rays form == restatement, volumes from tsdf_integrate on the
    base scene (9 x 13 x 21) rendered at 11 x 19, shared and per-image transforms and origins"""
    for per in (False, True):
        vol, vnp = _volumes(per_origin=per)
        r = _check(vol, vnp, (model, model), T_vc=rc.transforms(per), what=f"{tc.NAMES[model]} per={per}")
        rc.assert_not_vacuous(tc.NAMES[model], r)


def test_raw_rays_and_options():
    """rays that are not normalised, under a Spherical and an OPENCV tag (distance and z); min_weight above some weights; half the step;
    the second scene; the wave mappings and the full scan give the same bits"""
    from unidepth_amd import tsdf
    vol, vnp = _volumes()
    Ho, Wo = rc.SIZE
    rays = np.ones((2, 3, Ho, Wo), F)
    rays[:, 0] = ((np.arange(Wo, dtype=F) + F(0.5) - F(Wo / 2)) / F(14))[None, None, :]
    rays[:, 1] = ((np.arange(Ho, dtype=F) + F(0.5) - F(Ho / 2)) / F(14))[None, :, None]
    T = rc.transforms(True)
    r = _check(vol, vnp, (tc.SPHERICAL, tc.OPENCV), T_vc=T, rays=rays, what="raw rays")
    rc.assert_not_vacuous("raw rays", r)
    assert (r["depth"][0][r["valid"][0]] > r["points"][0, 2:3][r["valid"][0]]).all() and rc.same_bits(r["depth"][1], r["points"][1, 2:3])
    high = _check(vol, vnp, (tc.PINHOLE, tc.MEI), T_vc=T, min_weight=1.75, what="min_weight")
    base = _check(vol, vnp, (tc.PINHOLE, tc.MEI), T_vc=T, what="base")
    assert 0 < high["valid"].sum() < base["valid"].sum()
    _check(vol, vnp, (tc.PINHOLE, tc.MEI), T_vc=T, step=vnp["voxel"] / 2, what="half step")
    _check(vol, vnp, (tc.PINHOLE, tc.MEI), T_vc=T, far=24.0, what="long range")
    vol2, vnp2 = _volumes(second=True)
    rc.assert_not_vacuous("second", _check(vol2, vnp2, (tc.EUCM, tc.SPHERICAL), T_vc=T, what="second"))
    cam = tc.prepared(rc.params_for((tc.PINHOLE, tc.MEI), rc.SIZE), (tc.PINHOLE, tc.MEI))
    saved = dict(tsdf._RENDER_OPTIONS)
    try:
        res = []
        for patch in (0, 1):
            for full in (0, 1):
                tsdf._RENDER_OPTIONS.update(wave_patch=patch, full_scan=full)
                res.append(tsdf.tsdf_render(vol, cam, (13, 21), _dev(T), near=rc.NEAR, far=rc.FAR, **ALL))
    finally:
        tsdf._RENDER_OPTIONS.update(saved)
    for other in res[1:]:
        tc.host_program.assert_same(other, res[0], NAMES, "mapping / scan")
    assert bool(res[0][1].any())


def test_mixed_batches():
    """B = 3 batches mixing Pinhole, EUCM, Spherical and MEI; a batch with OPENCV and Fisheye624 members, which goes through
    unproject_camera's rays: equal to passing those rays, and to the restatement on them"""
    from unidepth_amd import tsdf, unproject
    vol, vnp = _volumes(B=3)
    T = rc.transforms(True, B=3)
    for models in ((tc.PINHOLE, tc.EUCM, tc.SPHERICAL), (tc.MEI, tc.SPHERICAL, tc.PINHOLE)):
        r = _check(vol, vnp, models, T_vc=T, what=str(models))
        assert all(r["valid"][b].any() for b in range(3))
    models = (tc.OPENCV, tc.FISHEYE624, tc.PINHOLE)
    r = _check(vol, vnp, models, T_vc=T, what="iterative", camera_form=False)
    cam = tc.prepared(rc.params_for(models, rc.SIZE), models)
    routed = tsdf.tsdf_render(vol, cam, rc.SIZE, _dev(T), near=rc.NEAR, far=rc.FAR, **ALL)
    rays = unproject.unproject_camera(None, cam, normalize=True, image_shape=rc.SIZE)
    tc.host_program.assert_same(routed, tsdf.tsdf_render(vol, cam, rc.SIZE, _dev(T), rays=rays, near=rc.NEAR, far=rc.FAR, **ALL), NAMES, "routed")
    rc.assert_same(_as_dict(routed, color=torch.uint8), r, "routed vs restatement", ("depth", "valid", "points", "normals", "color_u8"))
    assert all(r["valid"][b].any() for b in range(3))


@pytest.mark.parametrize("size", ((1, 1), (2, 3), (1, 63), (1, 64), (1, 65), (1, 257)))
def test_edge_image_sizes(size):
    vol, vnp = _volumes()
    r = _check(vol, vnp, (tc.PINHOLE, tc.EUCM), size=size, T_vc=rc.transforms(True), what=str(size))
    assert size == (1, 1) or r["valid"].any()


def test_edge_grids_ranges_and_batch_limit():
    """a 1 x 1 x 1 and a 1 x 1 x 2 grid; K = 1; near beyond the volume; B = 256 at 1 x 1"""
    rays = np.zeros((1, 3, 3, 5), F)
    rays[:, 2] = 1
    one = rc.planted((1, 1, 1), 0.5, (-0.25, -0.25, 0.75))
    r = _check(_upload(one), one, (tc.PINHOLE,), size=(3, 5), rays=rays, near=0.0, far=2.0, step=0.25, what="1x1x1")
    assert not r["valid"].any()
    two = rc.planted((2, 1, 1), 0.5, (-0.25, -0.25, 0.75))
    r = _check(_upload(two), two, (tc.PINHOLE,), size=(3, 5), rays=rays, near=0.0, far=2.0, step=0.25, what="1x1x2")
    assert r["valid"].all() and (r["depth"] == F(1.25)).all()
    vol, vnp = _volumes()
    T = rc.transforms(False)
    assert not _check(vol, vnp, (tc.PINHOLE,) * 2, T_vc=T, near=1.0, far=1.05, what="K=1")["valid"].any()
    assert not _check(vol, vnp, (tc.PINHOLE,) * 2, T_vc=T, near=6.0, far=9.0, what="near beyond")["valid"].any()
    big = rc.planted((4, 2, 2), 0.25, (-0.25, -0.25, 0.5), B=256)
    big["tsdf"] = (big["tsdf"] + (np.arange(256, dtype=F) / F(1024)).reshape(256, 1, 1, 1)).astype(F)
    rays = np.zeros((256, 3, 1, 1), F)
    rays[:, 2] = 1
    r = _check(_upload(big), big, tuple(rc.CLOSED[b % 4] for b in range(256)), size=(1, 1), rays=rays, near=0.0,
               far=2.0, step=0.125, what="B=256")
    assert r["valid"].all() and len(np.unique(r["depth"])) == 256


def test_optional_outputs():
    """each optional output on and off, both colour types: the outputs that are asked for do not depend on the others"""
    from unidepth_amd import tsdf
    vol, _ = _volumes()
    cam = tc.prepared(rc.params_for((tc.EUCM, tc.SPHERICAL), rc.SIZE), (tc.EUCM, tc.SPHERICAL))
    T = _dev(rc.transforms(True))
    kw = dict(near=rc.NEAR, far=rc.FAR)
    full = tsdf.tsdf_render(vol, cam, rc.SIZE, T, color_dtype=torch.float32, **ALL, **kw)
    assert [t.dtype for t in full] == [torch.float32, torch.bool] + [torch.float32] * 3
    assert [tuple(t.shape) for t in full] == [(2, 1) + rc.SIZE] * 2 + [(2, 3) + rc.SIZE] * 3
    for pts in (False, True):
        for nrm in (False, True):
            for col in (False, True):
                res = tsdf.tsdf_render(vol, cam, rc.SIZE, T, return_points=pts, return_normals=nrm, return_color=col, color_dtype=torch.float32, **kw)
                want = full[:2] + tuple(t for t, on in zip(full[2:], (pts, nrm, col)) if on)
                tc.host_program.assert_same(res, want, NAMES[:len(want)], f"{pts} {nrm} {col}")
    u8 = vol.render(cam, rc.SIZE, T, return_color=True, **kw)[2]
    assert u8.dtype == torch.uint8 and torch.equal(u8, torch.round(full[4]).clamp(0, 255).to(torch.uint8)) and bool(u8.any())
    # transforms as [4,4] / [B,4,4], a camera object
    T44 = torch.eye(4, device="cuda").repeat(2, 1, 1)
    T44[:, :3] = T
    tc.host_program.assert_same(tsdf.tsdf_render(vol, cam, rc.SIZE, T44, color_dtype=torch.float32, **ALL, **kw), full, NAMES, "4x4")


def test_known_answer():
    from unidepth_amd import tsdf
    s = tc.known_answer_scene()
    cam = tc.prepared(s["params"][0], s["models"][0])
    vol = tsdf.tsdf_integrate(None, _dev(s["depths"]), [cam], _dev(s["T"]), grid_shape=s["grid"], origin=_dev(s["origin"]), voxel_size=s["voxel"], trunc=s["trunc"])
    r = _check(vol, _numpy(vol), (tc.PINHOLE,), size=(16, 16), rays=rc.known_rays(), near=0.25, far=3.5, step=0.25, what="known answer")
    rc.check_known_answer(r["depth"], r["valid"], r["points"], r["normals"])


def test_special_values():
    """NaN, +-inf and -0.0 distances, NaN, inf and negative weights, NaN, zero and infinite ray components, a NaN and a mirrored
    transform, a singular Pinhole (the camera form): finite where valid, exactly 0 where not, equal to the restatement"""
    from unidepth_amd import tsdf, unproject
    vnp = rc.special_volume(_volumes()[1])
    T_cv, rays, params, models = rc.special_inputs()
    vol = _upload(vnp)
    T_vc = rc.invert(T_cv)                                                        # tsdf_render inverts it again: the NaN and the mirror stay
    want = rc.restate(vnp, models, rays, rc.invert(T_vc), min_weight=0.75)
    cam = tc.prepared(params, models)
    got = _as_dict(tsdf.tsdf_render(vol, cam, rc.SIZE, _dev(T_vc), rays=_dev(rays), near=rc.NEAR, far=rc.FAR, min_weight=0.75, **ALL), color=torch.uint8)
    rc.assert_same(got, want, "special", ("depth", "valid", "points", "normals", "color_u8"))
    rc.check_special(want)
    assert want["valid"][2].any() and not want["valid"][1].any()
    params = np.array(params)
    params[0, 0] = 0.0
    cam = tc.prepared(params, models)
    dirs = unproject.unproject_camera(None, cam, normalize=True, image_shape=rc.SIZE).cpu().numpy()
    want = rc.restate(vnp, models, dirs, rc.invert(T_vc), min_weight=0.75)
    got = _as_dict(tsdf.tsdf_render(vol, cam, rc.SIZE, _dev(T_vc), near=rc.NEAR, far=rc.FAR, min_weight=0.75, color_dtype=torch.float32, **ALL), color=torch.float32)
    rc.assert_same(got, want, "special, camera form", ("depth", "valid", "points", "normals", "color_f32"))
    rc.check_special(want)
    assert not want["valid"][0].any() and want["valid"][2].any()


# ---- the composition ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("second", (False, True))
def test_composition_equals_fused(second):
    """tsdf_render_composition == tsdf_render bit for bit on two small scenes (K = 28 and 14), a mixed batch, every output"""
    from unidepth_amd import tsdf
    vol, vnp = _volumes(second=second, per_origin=True)
    models = (tc.SPHERICAL, tc.MEI) if second else (tc.PINHOLE, tc.EUCM)
    cam = tc.prepared(rc.params_for(models, rc.SIZE), models)
    T = _dev(rc.transforms(True))
    for kw in (dict(color_dtype=torch.uint8), dict(color_dtype=torch.float32, min_weight=1.25)):
        got = tsdf.tsdf_render(vol, cam, rc.SIZE, T, near=rc.NEAR, far=rc.FAR, **ALL, **kw)
        want = tsdf.tsdf_render_composition(vol, cam, rc.SIZE, T, near=rc.NEAR, far=rc.FAR, **ALL, **kw)
        tc.host_program.assert_same(got, want, NAMES, f"composition {kw}")
        assert 0.1 < float(got[1].float().mean()) < 0.9
    got = tsdf.tsdf_render(vol, cam, rc.SIZE, near=rc.NEAR, far=rc.FAR, **ALL)
    tc.host_program.assert_same(got, tsdf.tsdf_render_composition(vol, cam, rc.SIZE, near=rc.NEAR, far=rc.FAR, **ALL), NAMES, "identity")
    assert bool(got[1].any())


# ---- guarded C-ABI ------------------------------------------------------------------------------------------------------------------

def test_guarded_render():
    """the entry point itself on guarded allocations: fp32 outputs off 16-byte boundaries, byte outputs at odd offsets, absent outputs
    untouched, guard bytes intact, two calls the same bits, and the bits the wrapper's"""
    from unidepth_amd import _lib, tsdf
    from unidepth_amd.ops import check, cur_stream, mk
    vol, _ = _volumes(per_origin=True)
    models = (tc.EUCM, tc.PINHOLE)
    T = _dev(rc.transforms(True))
    Ti = tsdf.invert_rigid(T).contiguous()
    for size in (rc.SIZE, (1, 65)):
        Ho, Wo = size
        hw = 2 * Ho * Wo
        cam = tc.prepared(rc.params_for(models, size), models)
        for f32 in (0, 1):
            want = tsdf.tsdf_render(vol, cam, size, T, near=rc.NEAR, far=rc.FAR, color_dtype=torch.float32 if f32 else torch.uint8, **ALL)
            for has in (dict(points=True, normals=True, color_out=True), dict(points=False, normals=False, color_out=False),
                        dict(points=False, normals=True, color_out=False)):
                bufs = dict(depth=_Out(hw, torch.float32, 1), valid=_Out(hw, torch.uint8, 3), points=_Out(3 * hw, torch.float32, 3),
                            normals=_Out(3 * hw, torch.float32, 1), color_out=_Out(3 * hw, torch.float32 if f32 else torch.uint8, 1))
                on = dict(depth=True, valid=True, **has)
                desc = mk(_lib.UdTsdfRender, tsdf=vol.tsdf, weight=vol.weight, color=vol.color, origin=vol.origin, T=Ti, params=cam.params, rays=None,
                          B=2, Ho=Ho, Wo=Wo, Nx=21, Ny=13, Nz=9, nT=2, n_origin=2, K=rc.n_samples(rc.NEAR, rc.FAR, vol.voxel_size), color_f32=f32,
                          full_scan=0, wave_patch=1, voxel_size_bits=tc.f32_bits(vol.voxel_size), near_bits=tc.f32_bits(rc.NEAR),
                          step_bits=tc.f32_bits(vol.voxel_size), min_weight_bits=tc.f32_bits(1.0),
                          **{k: (b.t.data_ptr() if on[k] else None) for k, b in bufs.items()})
                for b, m in enumerate(models):
                    desc.model[b] = m
                runs = []
                for _ in range(2):
                    check(_lib.lib.ud_tsdf_render(desc, cur_stream()), "ud_tsdf_render")
                    torch.cuda.synchronize()
                    runs.append({k: b.t.clone() for k, b in bufs.items() if on[k]})
                for k, b in bufs.items():
                    b.check(k, on[k])
                for k, w in zip(("depth", "valid", "points", "normals", "color_out"), want):
                    if on[k]:
                        assert torch.equal(tc.bits(runs[0][k]), tc.bits(runs[1][k])), k
                        assert torch.equal(tc.bits(runs[0][k]), tc.bits(w.reshape(-1))), (size, f32, k)


# ---- graph replay ------------------------------------------------------------------------------------------------------------------

def test_graph_replay_after_inputs_were_rewritten():
    """captured once with a PreparedCamera; replayed after the volume's contents, the transform and the camera rows were rewritten in
    place: each replay equals the eager call and the restatement"""
    from unidepth_amd import gtpoints, tsdf, unproject
    va, na = _volumes()
    other = _upload(dict(na, tsdf=np.where(na["tsdf"] < 1, na["tsdf"] * F(0.75), na["tsdf"]).astype(F), weight=np.roll(na["weight"], 1, axis=3)))
    vol = tsdf.TsdfVolume(va.tsdf.clone(), va.weight.clone(), va.color.clone(), va.origin.clone(), va.voxel_size)
    models = (tc.EUCM, tc.SPHERICAL)
    cam0 = tc.prepared(rc.params_for(models, rc.SIZE), models)
    cam = gtpoints.PreparedCamera(cam0.params.clone(), cam0.models)
    Ts = _dev(rc.transforms(True))
    T = Ts.clone()
    kw = dict(near=rc.NEAR, far=rc.FAR, **ALL)

    def fn():
        return tsdf.tsdf_render(vol, cam, rc.SIZE, T, **kw)
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
        src = other if k % 2 == 0 else va
        vol.tsdf.copy_(src.tsdf)
        vol.weight.copy_(src.weight)
        T.copy_(Ts.flip(0) if k % 2 == 0 else Ts)
        cam.params[0, :2].mul_(1.03 if k % 2 == 0 else 0.98)
        cam.params[1, 2:4].add_(0.25 if k % 2 == 0 else -0.125)
        graph.replay()
        torch.cuda.synchronize()
        tc.host_program.assert_same(static, fn(), NAMES, f"replay {k}")
        dirs = unproject.unproject_camera(None, cam, normalize=True, image_shape=rc.SIZE).cpu().numpy()
        want = rc.restate(_numpy(vol), models, dirs, rc.invert(T.cpu().numpy()))
        rc.assert_same(_as_dict(static, color=torch.uint8), want, f"replay {k} vs restatement", ("depth", "valid", "points", "normals", "color_u8"))
        assert bool(static[1].any())
