"""unproject_camera without a GPU (unidepth_amd/unproject.py, include/unidepth_hip.h UdCameraUnproject): the numpy fp32 restatement of
tools/make_golden_unproject.py against the reference's own Camera.unproject arrays and masks (tests/golden/unproject.npz) at the measured
bars, the conditions the generator promises, the functions of csrc/camera_models.h compiled for the host and driven in the two-pass
order under the host sanitizers (tests/unproj_host/unproj_host.cpp, a stand-alone program), the workspace query, every refusal of
ud_camera_unproject and the Python argument errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import host_program
import unproject_common as common

ROOT = common.ROOT
up, gp = common.up, common.gp
_case = common.case


def test_golden_has_every_case():
    g = common.golden()
    want = [f"{n}.{k}" for n in up.CASES for k in ("params", "models", "sum", "out", "mask", "steps")]
    want += [f"{k}.{n}" for n in up.MODEL_NAMES.values() for k in ("referr", "rterr")]
    assert sorted(g) == sorted(want)
    assert set(gp.CASES) <= set(up.CASES) and all(up.base_case(n) in gp.CASES for n in up.CASES)
    for name in up.CASES:
        c = _case(name)
        H, W = common.shape(name)
        B = len(c["models"])
        assert g[name + ".out"].dtype == np.float32 and g[name + ".out"].shape == (B, H * W, 3) and g[name + ".mask"].shape == (B, H * W)
        # the seeded inputs are the ones the stored outputs were made from, bit for bit (NaN included)
        assert list(g[name + ".sum"]) == [up.checksum(c["uv"]), up.checksum(c["depth"])]
        assert np.array_equal(g[name + ".params"], c["params"]) and list(g[name + ".models"]) == c["models"]
    assert os.path.getsize(up.GOLDEN) <= os.path.getsize(gp.GOLDEN)


def test_cases_reach_the_paths_they_are_there_for():
    for name in up.CASES:
        c = _case(name)
        H, W = common.shape(name)
        n_reg = up.n_regular(name)
        uv, size = c["uv"], np.array([W, H], np.float32)
        reg = uv[:, :n_reg]
        assert ((reg > 0) & (reg < size)).all() and (reg != np.rint(reg)).all(), name       # inside the image, off the integer grid
        out = uv[:, n_reg:n_reg + up.N_OUTSIDE]
        assert ((out >= -0.5 * size) & (out <= 1.5 * size)).all()
        for b, m in enumerate(c["models"]):
            want_nan = name.endswith("+nan") or m not in up.ITERATIVE
            assert np.isnan(uv[b]).any() == want_nan and np.isnan(uv[b, :-1]).sum() == 0, (name, b)
        d = c["depth"]
        assert (d == 0).any() and (d < 0).any() and ((d > 0) & (d < 1e-4)).any() and np.isnan(d).sum() == 1
        assert (d[:, :n_reg] >= 0.2).all()
    assert any(((np.asarray(_case(n)["uv"][:, up.n_regular(n):-1]) < 0).any() for n in up.CASES))     # some really are outside
    # a camera given to every image keeps one row
    p = _case("broadcast_opencv_9x29_b3")["params"]
    assert (p == p[0]).all()
    # EUCM with alpha above 0.5: a mask with both values, the exempt share below a tenth of the regular points of every image
    c = _case("eucm_9x29_b2")
    assert c["mask"][1].any() and not c["mask"][1].all()
    for name in up.CASES:
        c = _case(name)
        for b, m in enumerate(c["models"]):
            if m == up.EUCM:
                assert (~c["m64"][b, :up.n_regular(name)]).mean() < up.MASKED_SHARE, (name, b)
    # the NaN coordinate keeps an iterative image in its loop to the end
    st = _case("opencv_5x7_b2_tan+nan")["info"]["steps"]
    assert st[1] == 10


def test_residual_maxima_keep_clear_of_the_exit_threshold():
    """every OPENCV / Fisheye624 camera of every case, every iteration: the fp32 restatement's maximum |residual| over the image's own
    coordinate set lies outside [0.5e-3, 2e-3]; the iteration counts are the reference's"""
    g = common.golden()
    n, counts = 0, set()
    for name in up.CASES:
        c = _case(name)
        for b, m in enumerate(c["models"]):
            if m in up.ITERATIVE:
                maxima = c["info"].get("maxima", {}).get(b, [])
                assert gp.margins_ok(maxima), (name, b, maxima)
                assert c["info"].get("steps", {}).get(b, 0) == int(g[name + ".steps"][b]), (name, b)
                counts.add(int(g[name + ".steps"][b]))
                n += 1
            else:
                assert int(g[name + ".steps"][b]) == -1
    assert n >= 14 and {0, 1, 2, 10} <= counts


@pytest.mark.parametrize("name", list(up.CASES))
def test_fp32_restatement_within_measured_bar_of_reference(name):
    c, g = _case(name), common.golden()
    ref = g[name + ".out"]
    assert np.array_equal(np.isnan(ref), np.isnan(c["r64"]))
    w = common.assert_within_bars(c["raw"], ref, c["r64"], c["models"], common.bars(), name)
    for b, m in enumerate(c["models"]):                       # the masks, on every point: 2 where the class sets none
        assert np.array_equal(g[name + ".mask"][b], up.class_mask(m, c["mask"][b])), (name, b)
        assert np.array_equal(c["mask"][b], c["m64"][b])
    print(f"{name}: fp32 restatement uses {w:.3f} of the bar")


def test_bars_come_from_the_reference_error():
    g = common.golden()
    worst = {}
    for name in up.CASES:
        c = _case(name)
        e = up.ray_error(g[name + ".out"].astype(np.float64) - c["r64"], c["r64"])
        for b, m in enumerate(c["models"]):
            worst[m] = max(worst.get(m, 0.0), float(e[b].max()))
    for m, n in up.MODEL_NAMES.items():
        e = float(g["referr." + n])
        assert 0 < e < 1e-2 and up.bar(e) == max(4 * e, 8 * 2.0 ** -24)
        assert abs(worst[m] - e) <= 1e-6 * worst[m], n        # the fp64 restatement's libm may differ in its last bit
        assert float(g["rterr." + n]) > 0


def test_forms_of_the_restatement_agree_with_their_definitions():
    """normalize is raw / max(|raw|, 1e-4) and depth is the class's reconstruct rule on the raw ray, recomputed here from the raw output"""
    f32 = np.float32
    for name in ("mixed_37x53_b6", "pinhole_5x7_b2"):
        c = _case(name)
        with np.errstate(all="ignore"):
            raw, d = c["raw"], c["depth"][..., None]
            n = np.sqrt(raw[..., 0] * raw[..., 0] + raw[..., 1] * raw[..., 1] + raw[..., 2] * raw[..., 2])[..., None]
            assert np.array_equal(c["normalize"], raw / np.where(n < f32(1e-4), f32(1e-4), n), equal_nan=True)
            for b, m in enumerate(c["models"]):
                if m == up.SPHERICAL:
                    want = raw[b] * d[b]
                elif m == up.PINHOLE:
                    continue                                   # its division comes before the product: one rounding apart
                else:
                    z = raw[b, :, 2:]
                    want = raw[b] / np.where(z < f32(1e-4), f32(1e-4), z) * np.where(d[b] < f32(1e-4), f32(1e-4), d[b])
                assert np.array_equal(c["depth_form"][b], want, equal_nan=True), (name, b)


# ---- the header functions, compiled for the host with the sanitizers, in the two-pass order ------------------------------------------

@pytest.fixture(scope="module")
def unproj_host(tmp_path_factory):
    out = host_program.build(tmp_path_factory, "unproj_host")

    def run(model, form, row, uv, depth):
        N = uv.shape[0]
        rec = np.concatenate([uv, depth[:, None]], axis=1).astype(np.float32)
        k, rays, mask = host_program.run(out, [model, form, N] + [float(v).hex() for v in row], [rec.tobytes()], [4, 12 * N, N])
        return int(np.frombuffer(k, dtype=np.int32)[0]), np.frombuffer(rays, dtype=np.float32).reshape(N, 3), np.frombuffer(mask, dtype=np.uint8).astype(bool)
    return run


def _host_cameras():
    for name in up.CASES:                                     # from the static case table: nothing is computed while pytest collects
        _, _, cams, B = gp.CASES[up.base_case(name)]
        models = [m for m, _ in cams] * (B if len(cams) == 1 else 1)
        for b, m in enumerate(models):
            yield pytest.param(name, b, id=f"{name}-{b}-{up.MODEL_NAMES[m]}")


@pytest.mark.parametrize("name,b", list(_host_cameras()))
def test_header_functions_on_the_host_in_two_pass_order(unproj_host, name, b):
    """every camera of every case, all three forms: the host build equals the fp32 restatement bit for bit for Pinhole, EUCM, OPENCV and
    MEI (no libm beyond sqrt), within the model's measured bar for Spherical and Fisheye624 (their sin / cos / tan come from another
    libm); same masks, same iteration count"""
    c = _case(name)
    m = c["models"][b]
    for k, which in enumerate(common.FORMS):
        steps, rays, mask = unproj_host(m, k, c["params"][b], c["uv"][b], c["depth"][b])
        want = common.form(c, which)[b]
        assert steps == (c["info"]["steps"][b] if m in up.ITERATIVE else -1), (which, steps)
        assert np.array_equal(mask, c["mask"][b]), which
        assert common.same_specials(rays, want), which
        if m in (up.SPHERICAL, up.FISHEYE624):
            # two libms: the model's measured bar, |d| / max(|want|, 1e-4), the floor scaled with the depth in the depth form
            fin = np.isfinite(want)
            scale = np.maximum(np.abs(np.nan_to_num(c["depth"][b], nan=1.0)), 1.0)[:, None] if which == "depth" else 1.0
            den = np.maximum(np.abs(want.astype(np.float64)), 1e-4 * scale)
            assert (np.abs(rays.astype(np.float64) - want)[fin] <= (common.bars()[m] * den)[fin]).all(), which
        else:
            assert common.same_bits(rays, want), which


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_work_bytes_and_every_refusal():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    wb = _lib.lib.ud_camera_unproject_work_bytes
    assert wb(2, 0) == 0 and wb(2, 1) == 48 and wb(6, 2) == 96 and wb(256, 256) == 256 * 44      # 11 maxima per image, rounded up to 16 bytes
    for bad in ((0, 0), (_lib.UD_RECON_MAX_B + 1, 0), (2, 3), (2, -1)):
        assert wb(*bad) == -1, bad
    lib = _lib.lib
    assert lib.ud_camera_unproject(None, None) < 0 and "null descriptor" in lib.ud_last_error().decode()

    def call(**kw):
        d = _lib.UdCameraUnproject()
        base = dict(uv=16, params=16, depth=None, rays=16, valid=16, work=16, work_bytes=1 << 20, batch_stride=70, point_stride=2,
                    comp_stride=1, n_points=35, B=2, H=5, W=7, normalize=0, rays_rows=0)
        base.update(kw)
        models = base.pop("models", (1, 4))
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(models):
            d.model[b] = m
        return lib.ud_camera_unproject(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"),
                    (dict(n_points=-1), "bad sizes"), (dict(n_points=2 ** 31 - 256), "bad sizes"),
                    (dict(params=None), "null pointer"), (dict(rays=None), "null pointer"), (dict(work=None), "null pointer"),
                    (dict(work=24), "16-byte aligned"), (dict(work_bytes=47), "smaller than"),
                    (dict(models=(1, 0)), "model tag"), (dict(models=(7, 1)), "model tag"),
                    (dict(normalize=1, depth=16), "exclude"),
                    (dict(uv=None, n_points=34), "identity grid"), (dict(uv=None, n_points=36), "identity grid"),
                    (dict(point_stride=0), "bad strides"), (dict(comp_stride=0), "bad strides"), (dict(batch_stride=-1), "bad strides"),
                    (dict(comp_stride=-1), "bad strides")):
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    # nothing to do is not a refusal, and asks for no device either
    assert call(n_points=0)[0] == 0 and call(n_points=0, models=(1, 2), work=None)[0] == 0


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, unproject
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    uv = torch.rand(2, 2, 5, 7)
    rows = torch.rand(2, 11, 2)
    f = unproject.unproject_camera
    for bad in (torch.rand(2, 3, 5, 7), torch.rand(2, 11, 3), torch.rand(5, 7), torch.ones(2, 2, 5, 7, dtype=torch.int32), torch.rand(0, 2, 5, 7), "uv"):
        with pytest.raises(ValueError):
            f(bad, K)
    with pytest.raises(ValueError, match="image_shape"):
        f(None, K)
    for shp in ((0, 7), (5,), "hw"):
        with pytest.raises(ValueError, match="image_shape"):
            f(None, K, image_shape=shp)
    with pytest.raises(ValueError, match="exclude"):
        f(uv, K, depth=torch.ones(2, 1, 5, 7), normalize=True)
    for bad_depth in (torch.ones(2, 1, 5, 6), torch.ones(2, 35, dtype=torch.int32), torch.ones(2, 2, 5, 7)):
        with pytest.raises(ValueError, match="depth"):
            f(uv, K, depth=bad_depth)
    with pytest.raises(ValueError, match="depth"):
        f(rows, K, depth=torch.ones(2, 1, 11))
    with pytest.raises(ValueError):
        f(uv, K, depth=torch.ones(3, 1, 5, 7))                                    # uv of 2 images, depth of 3
    with pytest.raises(ValueError):
        f(uv, cameras.BatchCamera([cameras.Pinhole(K)] * 3))                      # uv of 2 images, 3 cameras
    with pytest.raises(ValueError):
        f(torch.rand(3, 2, 5, 7), K.expand(2, 3, 3))
    with pytest.raises(NotImplementedError):
        f(uv, object())
    for bad_shapes in ((5,), (1, 2, 5, 7), (0, 5, 7), "x"):
        with pytest.raises(ValueError, match="shapes"):
            unproject.get_rays(K, bad_shapes)
    # well-formed arguments on the CPU: the HIP kernels are the only implementation
    eucm = cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))
    for cam in (K, cameras.Pinhole(K), cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12)), cameras.BatchCamera([cameras.Pinhole(K), eucm])):
        for args, kw in (((uv,), {}), ((rows,), {}), ((uv[:1],), {}), ((uv,), dict(depth=torch.ones(2, 5, 7))), ((rows,), dict(normalize=True, return_mask=True))):
            with pytest.raises(RuntimeError, match="GPU"):
                f(*args, cam, **kw)
        with pytest.raises(RuntimeError, match="GPU"):
            cameras.as_camera(cam).unproject(uv) if not isinstance(cam, torch.Tensor) else f(uv, cam)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            f(None, K, image_shape=(5, 7))
        with pytest.raises(RuntimeError, match="GPU"):
            eucm.get_rays((5, 7))
    for cls in (cameras.Pinhole, cameras.EUCM, cameras.Spherical, cameras.OPENCV, cameras.Fisheye624, cameras.MEI, cameras.BatchCamera):
        assert callable(cls.unproject) and callable(cls.get_rays) and cls.unprojection_mask is None
    for name in ("unproject_camera", "get_rays"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(unproject, name)
