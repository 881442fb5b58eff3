"""tsdf_render without a GPU (unidepth_amd/tsdf.py, include/unidepth_hip.h UdTsdfRender): the per-ray function of csrc/tsdf_ray.h compiled for
the host and run under the host sanitizers (tests/tsdf_render_host/tsdf_render_host.cpp, a stand-alone program), the clipped against the
full scan inside the program and the full scan against the numpy restatement of tests/tsdf_render_common.py, bit for bit in every output;
the conditions no scene may miss; the known answer and the special values; every refusal of the entry point and
the Python argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_common as tc
import tsdf_render_common as rc

F = np.float32


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    return rc.build_hosts(tmp_path_factory)


def _both(hosts, vol, models, size=rc.SIZE, T_vc=None, rays=None, what="", vacuous=True, **kw):
    """the host program (camera form, or the rays form with `rays`) and the restatement on the program's directions, bit for bit ->
    the restatement's result"""
    T_cv = None if T_vc is None else rc.invert(T_vc)
    params = rc.params_for(models, size)
    h = rc.host_render(hosts[1], vol, models, params, size, T_cv, rays, **kw)
    if rays is not None:
        assert rc.same_bits(h["dirs"], np.asarray(rays, F))
    r = rc.restate(vol, models, h["dirs"], T_cv, **kw)
    assert r["K"] == h["K"]
    rc.assert_same(h, r, what)
    if vacuous:
        rc.assert_not_vacuous(what, r)
    return r


@pytest.mark.parametrize("model", rc.CLOSED + ("rays",))
def test_host_equals_restatement(hosts, model):
    """each closed-form model and the rays form (the rays of a Pinhole, not normalised, with a Spherical tag: the depth is the distance),
    on the base scene, shared and per-image transforms and origins, with and without colours"""
    for per in (False, True):
        vol = rc.volume(hosts[0], colour=True, per_origin=per)
        T = rc.transforms(per)
        if model == "rays":
            Ho, Wo = rc.SIZE
            rays = np.ones((2, 3, Ho, Wo), F)
            rays[:, 0] = ((np.arange(Wo, dtype=F) + F(0.5) - F(Wo / 2)) / F(14))[None, None, :]
            rays[:, 1] = ((np.arange(Ho, dtype=F) + F(0.5) - F(Ho / 2)) / F(14))[None, :, None]
            r = _both(hosts, vol, (tc.SPHERICAL, tc.OPENCV), T_vc=T, rays=rays, what=f"rays per={per}")
            z = r["points"][:, 2:3]
            assert (r["depth"][0][r["valid"][0]] > z[0][r["valid"][0]]).all() and rc.same_bits(r["depth"][1], z[1])
        else:
            r = _both(hosts, vol, (model, model), T_vc=T, what=f"{tc.NAMES[model]} per={per}")
        assert r["color_u8"].any() and (np.abs(r["normals"]).sum(axis=1)[r["valid"][:, 0]] > 0).all()
        plain = _both(hosts, rc.volume(hosts[0], colour=False, per_origin=per), (model, model) if model != "rays" else (tc.SPHERICAL, tc.OPENCV),
                      T_vc=T, rays=rays if model == "rays" else None, what="no colour")
        rc.assert_same(plain, r, "colour changes nothing else", ("depth", "valid", "points", "normals"))


def test_host_options_and_second_scene(hosts):
    """min_weight 1 and a value above some weights; step = voxel and voxel / 2; the second scene; a mixed batch"""
    vol = rc.volume(hosts[0])
    T = rc.transforms(True)
    models = (tc.PINHOLE, tc.MEI)
    base = _both(hosts, vol, models, T_vc=T, what="base")
    high = _both(hosts, vol, models, T_vc=T, min_weight=1.75, what="min_weight", vacuous=False)
    assert (vol["weight"] < 1.75).any() and high["valid"].sum() < base["valid"].sum() and high["valid"].any()
    half = _both(hosts, vol, models, T_vc=T, step=vol["voxel"] / 2, what="half step")
    assert half["K"] == 2 * base["K"] - 1 and not rc.same_bits(half["depth"], base["depth"])
    second = rc.volume(hosts[0], second=True)
    _both(hosts, second, (tc.EUCM, tc.SPHERICAL), T_vc=T, what="second")
    # the box covers under a tenth of [near, far]
    far = rc.restate(vol, models, rc.host_render(hosts[1], vol, models, rc.params_for(models, rc.SIZE), rc.SIZE, rc.invert(T), far=24.0)["dirs"],
                     rc.invert(T), far=24.0)
    assert far["K"] > 10 * 21 and rc.same_bits(far["depth"], base["depth"])
    _both(hosts, vol, models, T_vc=T, far=24.0, what="long range")


EDGE_SIZES = ((1, 1), (2, 3), (1, 63), (1, 64), (1, 65), (1, 257))


@pytest.mark.parametrize("size", EDGE_SIZES)
def test_host_edge_image_sizes(hosts, size):
    vol = rc.volume(hosts[0])
    r = _both(hosts, vol, (tc.PINHOLE, tc.EUCM), size=size, T_vc=rc.transforms(True), what=str(size), vacuous=False)
    assert size == (1, 1) or r["valid"].any()


def test_host_edge_grids_and_ranges(hosts):
    """a 1 x 1 x 1 and a 1 x 1 x 2 grid; K = 1 (nothing valid); near beyond the volume; rays parallel to a face, rays that start inside
    the box, rays that miss it"""
    Ho, Wo = 3, 5
    rays = np.zeros((1, 3, Ho, Wo), F)
    rays[:, 2] = 1
    # one voxel: only a sample exactly at its centre lies in the grid; the distance there is 0 at every sample: no crossing
    one = rc.planted((1, 1, 1), 0.5, (-0.25, -0.25, 0.75))
    r = _both(hosts, one, (tc.PINHOLE,), size=(Ho, Wo), rays=rays, near=0.0, far=2.0, step=0.25, what="1x1x1", vacuous=False)
    assert not r["valid"].any() and r["outside"] == 0
    # two voxels along z with centres 1.0 (+0.25) and 1.5 (-0.25): the ray along the axis crosses at z = 1.25
    two = rc.planted((2, 1, 1), 0.5, (-0.25, -0.25, 0.75))
    r = _both(hosts, two, (tc.PINHOLE,), size=(Ho, Wo), rays=rays, near=0.0, far=2.0, step=0.25, what="1x1x2", vacuous=False)
    assert r["valid"].all() and (r["depth"] == F(1.25)).all() and (r["normals"][:, 2] == -1).all() and (r["color_f32"] == 0).all()
    vol = rc.volume(hosts[0])
    T = rc.transforms(False)
    r = _both(hosts, vol, (tc.PINHOLE,) * 2, T_vc=T, near=1.0, far=1.05, what="K=1", vacuous=False)
    assert r["K"] == 1 and not r["valid"].any()
    r = _both(hosts, vol, (tc.PINHOLE,) * 2, T_vc=T, near=6.0, far=9.0, what="near beyond", vacuous=False)
    assert not r["valid"].any() and r["outside"] == r["valid"].size
    # identity transform: the rays along +z are parallel to four faces (two zero components); some start inside the box, some miss it
    grid = rc.planted((8, 6, 10), 0.25, (-1.25, -0.75, -0.5), plane=1.0)
    rays = np.zeros((1, 3, 4, 9), F)
    rays[:, 2] = 1
    rays[0, 0, 1] = np.linspace(-0.9, 0.9, 9)                                     # a fan in x, y = 0 exactly
    rays[0, 1, 2] = 0.5                                                           # oblique in y
    rays[0, :, 3] = np.array([1.0, 0.0, 0.0], F)[:, None]                         # along +x at z = 0: never in front of the plane's crossing
    for near in (0.0, 0.3):
        r = _both(hosts, grid, (tc.PINHOLE,), size=(4, 9), rays=rays, near=near, far=4.0, step=0.25, what=f"faces near={near}", vacuous=False)
        assert r["valid"][0, 0, 0].all() and (r["depth"][0, 0, 0] == F(1.0)).all() and r["outside"] == 0
    # moved off the grid in x: every ray of rows 0 and 2 misses the box
    moved = np.zeros((1, 3, 4), F)
    moved[0, :, :3] = np.eye(3)
    moved[0, 0, 3] = 5.0
    r = _both(hosts, grid, (tc.PINHOLE,), size=(4, 9), T_vc=moved, rays=rays, near=0.0, far=4.0, step=0.25, what="missing", vacuous=False)
    assert r["outside"] >= 18 and not r["valid"][0, 0, 0].any()


def test_host_known_answer(hosts):
    vol = rc.known_answer_volume(hosts[0])
    r = _both(hosts, vol, (tc.PINHOLE,), size=(16, 16), rays=rc.known_rays(), near=0.25, far=3.5, step=0.25, what="known answer", vacuous=False)
    rc.check_known_answer(r["depth"], r["valid"], r["points"], r["normals"])


def test_host_special_values(hosts):
    """NaN, +-inf and -0.0 distances, NaN, inf and negative weights, NaN, zero and infinite ray components, a NaN and a mirrored
    transform, a singular Pinhole: finite where valid, exactly 0 where not, no sanitizer report, the clip equal to the full scan"""
    vol, T_cv, rays, params, models = rc.special_case(hosts[0])
    for kw in (dict(rays=rays), dict(rays=None)):
        p = np.array(params)
        p[0, 0] = 0.0                                                             # fx = 0: every direction of image 0 is NaN or inf
        h = rc.host_render(hosts[1], vol, models, p, rc.SIZE, T_cv, min_weight=0.75, **kw)
        r = rc.restate(vol, models, h["dirs"], T_cv, min_weight=0.75)
        rc.assert_same(h, r, "special")
        rc.check_special(r)
        assert not r["valid"][1].any()                                            # the NaN transform
        assert r["valid"][2].any() and (kw["rays"] is None) == (not r["valid"][0].any())


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_of_render():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_tsdf_render(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    nan, inf, neg, zero = (tc.f32_bits(v) for v in (float("nan"), float("inf"), -0.5, 0.0))

    def call(**kw):
        d = _lib.UdTsdfRender()
        base = dict(tsdf=16, weight=16, color=None, origin=16, T=16, params=16, rays=None, depth=16, valid=16, points=None, normals=None,
                    color_out=None, B=2, Ho=5, Wo=7, Nx=4, Ny=5, Nz=6, nT=1, n_origin=1, K=10, color_f32=0, full_scan=0, wave_patch=0,
                    voxel_size_bits=tc.f32_bits(0.1), near_bits=tc.f32_bits(0.5), step_bits=tc.f32_bits(0.1), min_weight_bits=tc.f32_bits(1.0))
        base.update(kw)
        models = base.pop("models", (1, 6))
        for k, v in base.items():
            setattr(d, k, v)
        for k, m in enumerate(models):
            d.model[k] = m
        return lib.ud_tsdf_render(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in (
            (dict(B=0), "bad sizes"), (dict(B=-1), "bad sizes"), (dict(B=257), "bad sizes"), (dict(Ho=0), "bad sizes"), (dict(Wo=-1), "bad sizes"),
            (dict(Nx=0), "bad sizes"), (dict(Ny=-1), "bad sizes"), (dict(Nz=0), "bad sizes"),
            (dict(Ho=1 << 16, Wo=1 << 15), "too large"), (dict(Ho=1 << 15, Wo=1 << 15), "too large"), (dict(Ho=2 ** 31 - 1, Wo=2 ** 31 - 1), "too large"),
            (dict(Nx=1 << 11, Ny=1 << 10, Nz=1 << 10), "too large"), (dict(Nx=2 ** 31 - 256, Ny=1, Nz=1), "too large"),
            (dict(Nx=1 << 16, Ny=1 << 16, Nz=1 << 16), "too large"),
            (dict(tsdf=None), "null pointer"), (dict(weight=None), "null pointer"), (dict(origin=None), "null pointer"),
            (dict(depth=None), "null pointer"), (dict(valid=None), "null pointer"),
            (dict(color_out=16), "color_out needs"),
            (dict(nT=0), "nT"), (dict(nT=3), "nT"), (dict(n_origin=0), "n_origin"), (dict(n_origin=3), "n_origin"),
            (dict(voxel_size_bits=nan), "voxel_size"), (dict(voxel_size_bits=inf), "voxel_size"), (dict(voxel_size_bits=neg), "voxel_size"),
            (dict(voxel_size_bits=zero), "voxel_size"), (dict(step_bits=nan), "step"), (dict(step_bits=inf), "step"), (dict(step_bits=neg), "step"),
            (dict(step_bits=zero), "step"), (dict(near_bits=nan), "near"), (dict(near_bits=inf), "near"), (dict(near_bits=neg), "near"),
            (dict(min_weight_bits=nan), "min_weight"),
            (dict(K=0), "K (the number"), (dict(K=-3), "K (the number"), (dict(K=16385), "K (the number"),
            (dict(models=(1, 0)), "model tag"), (dict(models=(7, 2)), "model tag"),
            (dict(models=(1, 4)), "needs rays"), (dict(models=(5, 1)), "needs rays"),
            (dict(params=None), "params is needed")):
        rc_, err = call(**kw)
        assert rc_ == -1 and msg in err and err.startswith("ud_tsdf_render: "), (kw, rc_, err)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, tsdf
    K = torch.tensor([[9.0, 0, 9.5], [0, 9.0, 5.5], [0, 0, 1]])
    cpu = tsdf.TsdfVolume(torch.ones(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), None, torch.zeros(1, 3), 0.1)
    for f in (tsdf.tsdf_render, tsdf.tsdf_render_composition, cpu.render):
        fn = "tsdf_render" if f == cpu.render else f.__name__
        call = (lambda *a, **kw: f(*a, **kw)) if f == cpu.render else (lambda *a, **kw: f(cpu, *a, **kw))    # noqa: E731
        with pytest.raises(ValueError, match=f"{fn}: volume.tsdf must be a contiguous fp32 GPU tensor"):
            call(K, (5, 7), near=0.5, far=2.0)
    with pytest.raises(ValueError, match="tsdf_render: volume must be a TsdfVolume"):
        tsdf.tsdf_render(torch.ones(2, 3, 4, 5), K, (5, 7), near=0.5, far=2.0)
    # past the volume check without a GPU: a volume whose tensors only claim to be there
    fake = tsdf.TsdfVolume(torch.ones(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), None, torch.zeros(1, 3), 0.1)
    real = tsdf._check_volume
    tsdf._check_volume = lambda fn, v: (2, 3, 4, 5, 0.1, tc.f32_bits(0.1))
    try:
        for f in (tsdf.tsdf_render, tsdf.tsdf_render_composition):
            fn = f.__name__

            def bad(match, *args, exc=ValueError, **kw):
                kw = {**dict(near=0.5, far=2.0), **kw}
                with pytest.raises(exc, match=match):
                    f(fake, *(args or (K, (5, 7))), **kw)
            for size in ((5,), (0, 7), 7, None, ("a", 1)):
                bad(f"{fn}: size", K, size)
            bad(f"{fn}: camera", None, (5, 7))
            bad(f"{fn}: camera of 3 images", cameras.BatchCamera([cameras.Pinhole(K)] * 3), (5, 7))
            for t in (torch.eye(4).double(), torch.eye(3), torch.eye(4).repeat(3, 1, 1), "T", torch.rand(2, 2, 3, 4)):
                bad(f"{fn}: transforms", K, (5, 7), t)
            for r in (torch.rand(2, 3, 5, 6), torch.rand(2, 3, 5, 7).double(), torch.rand(1, 3, 5, 7), torch.rand(2, 2, 5, 7), "r"):
                bad(f"{fn}: rays", rays=r)
            for v in (-0.1, float("nan"), float("inf"), "x", True, None):
                bad(f"{fn}: near", near=v)
            for v in (float("nan"), float("inf"), "x", None, 0.25, True):
                bad(f"{fn}: far", far=v)
            for v in (0, -0.1, float("nan"), float("inf"), "x", True):
                bad(f"{fn}: step", step=v)
            for v in (float("nan"), "x", None, True):
                bad(f"{fn}: min_weight", min_weight=v)
            bad(f"{fn}: 16386 samples", near=0.0, far=16385.0, step=1.0)
            bad(f"{fn}: [0-9]+ samples", far=1e6)
            bad(f"{fn}: color_dtype", color_dtype=torch.float16)
            bad(f"{fn}: return_color needs", return_color=True)
            bad(f"{fn}: unsupported sizes", K, (1 << 15, 1 << 15))
            # well-formed arguments on the CPU: the HIP kernel is the only implementation
            for args, kw in (((K, (5, 7)), {}), ((K, (5, 7), torch.eye(4)), dict(step=0.05, min_weight=0)),
                             ((cameras.EUCM(torch.tensor([9.0, 9, 9.5, 5.5, 0.5, 1.0])), (5, 7), torch.eye(4)[:3].repeat(2, 1, 1)),
                              dict(rays=torch.rand(2, 3, 5, 7), return_points=True, return_normals=True, color_dtype=torch.float32))):
                bad("GPU", *args, exc=RuntimeError, **kw)
    finally:
        tsdf._check_volume = real
    for name in ("tsdf_render", "tsdf_render_composition"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(tsdf, name)
    doc = tsdf.tsdf_render.__doc__
    assert "VOLUME (world) TO CAMERA" in doc and "PreparedCamera" in doc and "unproject_camera" in doc
