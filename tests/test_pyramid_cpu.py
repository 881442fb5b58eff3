"""depth_pyramid and the pyramid cameras without a GPU (unidepth_amd/pyramid.py, include/unidepth_hip.h UdDepthPyramid): the functions of
csrc/pyramid_point.h compiled for the host and run under the host sanitizers (tests/pyramid_host/pyramid_host.cpp, a stand-alone program)
against the numpy fp32 restatement, bit for bit -- the sizes 1x1 .. 67x129, the radii 0 / 1 / 4, mask and weights on and off, the special
values, the step edge and the constant plane; the two shares that show that the scenes take both sides of the range gate and of the level
gate; the tables of the filter against fp64 numpy; the rows of pyramid_cameras through tests/proj_host; the C-ABI's descriptor, every
refusal of the entry point and the Python argument errors.  Shared helpers: tests/pyramid_common.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import host_program
import pyramid_common as pc
import tsdf_common as tc

F = np.float32
SIZES = ((1, 1, 1), (2, 2, 2), (8, 8, 4), (33, 65, 3), (67, 129, 3))          # H, W, levels


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pc.build_host(tmp_path_factory)


def _filter(radius, sigma_range=pc.SIGMA_RANGE):
    if radius == 0:
        return dict(radius=0)
    ws, wr, inv_bin = pc.tables(radius, pc.SIGMA_SPACE, sigma_range)
    return dict(radius=radius, ws=ws, wr=wr, inv_bin=inv_bin)


def _same(got, want, what):
    for kind, g, w in (("depth", got[0], want[0]), ("weights", got[1], want[1])):
        assert (g is None) == (w is None), (what, kind)
        for l in range(len(g or ())):
            assert pc.same_bits(g[l], w[l]), (what, kind, l, int((g[l].view(np.int32) != w[l].view(np.int32)).sum()))


@pytest.mark.parametrize("H,W,levels", SIZES)
@pytest.mark.parametrize("radius", (0, 1, 4))
def test_header_on_the_host_against_the_restatement(host, H, W, levels, radius):
    """every size and radius, mask and weights on and off, a finite and an infinite gate: the host build of pyramid_point.h and the
    numpy restatement agree in every bit of every level"""
    s = pc.scene(2, H, W)
    for use_mask, use_w, gate in ((0, 0, np.inf), (1, 1, pc.GATE), (1, 0, pc.GATE), (0, 1, np.inf)):
        kw = dict(mask=s["mask"] if use_mask else None, weights=s["weights"] if use_w else None, gate=gate, **_filter(radius))
        _same(pc.host_run(host, s["depth"], levels, **kw), pc.restate(s["depth"], levels, **kw), (H, W, levels, radius, use_mask, use_w))


def test_scenes_take_both_sides_of_both_gates():
    """asserted on the restatement, so that no scene hides a branch: between 10 % and 90 % of the used taps fall in the last range bin,
    and between 10 % and 90 % of the level-1 blocks exclude at least one live member through the gate"""
    for H, W, levels in SIZES[3:]:
        for radius in (1, 4):
            s, st = pc.scene(2, H, W), {}
            pc.restate(s["depth"], levels, mask=s["mask"], weights=s["weights"], gate=pc.GATE, stats=st, **_filter(radius))
            print(f"{H}x{W} r={radius}: last bin {st['last_bin']:.3f}, gated blocks {st['gated']:.3f}")
            assert 0.1 <= st["last_bin"] <= 0.9 and 0.1 <= st["gated"] <= 0.9, st


@pytest.mark.parametrize("radius", (0, 1, 4))
def test_special_values(host, radius):
    """NaN, +-inf, negatives, -0, subnormals, 1e38 beside 1e-3 (delta * inv_bin overflows with sigma_range 1e-3): host and restatement
    agree bit for bit, every pixel that is not live is +0 at level 0, and no level holds a NaN"""
    s = pc.special_scene()
    f = _filter(radius, sigma_range=1e-3)
    if radius:
        with np.errstate(all="ignore"):
            assert np.isinf(F(1e38) * f["inv_bin"])
    for gate in (np.inf, 0.0, 0.5):
        kw = dict(mask=s["mask"], weights=s["weights"], gate=gate, **f)
        got, want = pc.host_run(host, s["depth"], 3, **kw), pc.restate(s["depth"], 3, **kw)
        _same(got, want, ("special", radius, gate))
        d, w = s["depth"], s["weights"]
        with np.errstate(all="ignore"):
            live = (s["mask"] != 0) & (d > 0) & (d < np.inf) & (w > 0) & (w < np.inf)
        assert not live.reshape(-1)[:6].any() and live[0, 0, 6:12].all() and not live[0, 1, :5].any()
        assert pc.same_bits(got[0][0][~live], np.zeros(int((~live).sum()), F)) and pc.same_bits(got[1][0][~live], np.zeros(int((~live).sum()), F))
        if radius == 0:
            assert pc.same_bits(got[0][0][live], d[live]) and pc.same_bits(got[1][0][live], w[live])
        assert all(not np.isnan(x).any() for maps in got for x in maps)


def test_step_edge_has_no_phantom_depth(host):
    """a clean step between 1.0 and 4.0 (powers of two, so the filter of a constant side is exact): with the gate below the step every pixel of every level is exactly one of the two surfaces
    (the nearer one in a block that straddles the edge); with an infinite gate the straddling blocks average to 2.5"""
    s = pc.step_scene(16, 24)
    for radius in (0, 1):
        kw = dict(gate=0.5, **_filter(radius, sigma_range=0.1))
        got = pc.host_run(host, s["depth"], 4, **kw)
        _same(got, pc.restate(s["depth"], 4, **kw), ("step", radius))
        for l, x in enumerate(got[0]):
            assert set(np.unique(x)) <= {F(1.0), F(4.0)}, (radius, l, np.unique(x))
        assert got[0][1][0, 0, 6] == F(1.0)                              # the block over columns 12, 13: the edge lies between them
    free = pc.host_run(host, s["depth"], 2, gate=np.inf)[0][1]
    assert free[0, 0, 6] == F(2.5)


def test_constant_plane_stays_constant(host):
    """the known answer: a plane of 2.0 (a power of two: every weighted sum is exactly twice the sum of the weights) is 2.0 at every
    pixel of every level, and the weights of a constant weight map stay that constant"""
    d, w = np.full((1, 33, 65), 2.0, F), np.full((1, 33, 65), 0.75, F)
    for radius in (0, 1, 4):
        got_d, got_w = pc.host_run(host, d, 4, weights=w, gate=0.0, **_filter(radius))
        for l in range(4):
            assert pc.same_bits(got_d[l], np.full((1, 33 >> l, 65 >> l), 2.0, F)) and pc.same_bits(got_w[l], np.full((1, 33 >> l, 65 >> l), 0.75, F))


# ---- the tables ----------------------------------------------------------------------------------------------------------------------

def test_filter_tables_against_fp64_numpy():
    from unidepth_amd import pyramid
    for radius, ss, sr in ((0, 1.0, 0.05), (1, 0.8, 0.02), (2, 1.5, 0.05), (4, 3.0, 1e-3), (4, 2.0, 7.5)):
        ws, wr, inv_bin = pyramid.filter_tables(radius, ss, sr)
        want = pc.tables(radius, ss, sr)
        assert pc.same_bits(ws, want[0]) and pc.same_bits(wr, want[1]) and pc.same_bits(np.asarray(inv_bin), np.asarray(want[2]))
        assert ws.shape == ((2 * radius + 1) ** 2,) and wr.shape == (256,) and ws[len(ws) // 2] == 1 and wr[0] > 0 and wr[255] == 0 and wr[254] > 0
        assert abs(float(inv_bin) * 3 * sr / 256 - 1) < 1e-6
    # ws[centre] = exp(0) and wr[0] = exp(-(1.5 / 256)^2 / 2) are positive by construction; what can fail is the bin width in fp32
    with pytest.raises(ValueError, match="prepare_depth_filter: .*not a positive fp32"):
        pyramid.filter_tables(1, 1.0, 1e-42)


# ---- the level cameras ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def proj_host(tmp_path_factory):
    out = host_program.build(tmp_path_factory, "proj_host", sanitize=False)

    def run(model, H, W, row, xyz):
        n = len(xyz)
        uv, depth, inside = host_program.run(out, [model, H, W, n] + [float(v).hex() for v in row], [np.ascontiguousarray(xyz, F).tobytes()],
                                             [8 * n, 4 * n, n])
        return np.frombuffer(uv, F).reshape(n, 2)
    return run


def test_level_rows_project_to_halved_coordinates(proj_host):
    """pyramid_cameras' rows through the host build of camera_models.h: uv_l == uv_0 / 2^l bit for bit for all six models; the points
    lie in front of the camera inside a 96 x 128 image, away from subnormal coordinates"""
    from unidepth_amd import pyramid
    H, W, f = 96, 128, 70.0
    g = np.random.RandomState(77)
    xyz = np.stack([g.uniform(-0.8, 0.8, 400), g.uniform(-0.6, 0.6, 400), g.uniform(1.0, 3.0, 400)], axis=1).astype(F)
    models = (1, 2, 3, 4, 5, 6)
    rows = np.stack([tc.row_for(m, H, W, f) for m in models])
    levels = pyramid.level_rows(torch.from_numpy(rows), models, 4)
    assert len(levels) == 4 and torch.equal(levels[0], torch.from_numpy(rows))
    sph = levels[1][2].numpy()
    assert sph[4] == (W + 1) / 2 and sph[5] == (H + 1) / 2 and sph[6] == rows[2, 6] and sph[7] == rows[2, 7]
    for b, m in enumerate(models):
        uv0 = proj_host(m, H, W, rows[b], xyz)
        assert np.isfinite(uv0).all() and (np.abs(uv0) > 1e-3).all()
        for l in range(1, 4):
            uvl = proj_host(m, H >> l, W >> l, levels[l][b].numpy(), xyz)
            assert pc.same_bits(uvl, (uv0 / F(2 ** l)).astype(F)), (m, l, np.abs(uvl - uv0 / 2 ** l).max())
    # a plain scaling of the Spherical row's W and H (the slip the identity excludes) misses by a quarter of a pixel and more
    wrong = rows[2].copy()
    wrong[:6] *= 0.5
    assert np.abs(proj_host(3, H >> 1, W >> 1, wrong, xyz) - proj_host(3, H, W, rows[2], xyz) / 2).max() >= 0.2


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------------

def test_pyramid_descriptor_size_and_build_flags():
    from unidepth_amd import _lib
    assert C.sizeof(_lib.UdDepthPyramid) == 5 * 8 + 8 * 8 + 8 * 4
    build = open(os.path.join(host_program.ROOT, "unidepth_amd", "csrc", "build.sh")).read()
    assert re.search(r"-ffp-contract=off [^\n]*-c pyramid\.hip", build)


def test_every_refusal():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_depth_pyramid(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    nan32, inf32, neg32 = pc.f32_bits(float("nan")), pc.f32_bits(float("inf")), pc.f32_bits(-0.5)

    def call(**kw):
        d = _lib.UdDepthPyramid()
        base = dict(depth=16, mask=None, weights=None, ws=16, wr=16, B=2, H=9, W=12, levels=3, radius=2, tile=0, gate_bits=inf32,
                    inv_bin_bits=pc.f32_bits(100.0))
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        d.out_depth[0] = 16
        return lib.ud_depth_pyramid(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in (
            (dict(B=0), "bad sizes"), (dict(B=-1), "bad sizes"), (dict(B=257), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-3), "bad sizes"),
            (dict(H=3), "bad sizes"), (dict(W=3), "bad sizes"), (dict(levels=4, H=7, W=64), "bad sizes"), (dict(H=1 << 16, W=1 << 15), "bad sizes"),
            (dict(levels=0), "levels"), (dict(levels=5), "levels"), (dict(levels=-1), "levels"),
            (dict(radius=-1), "radius"), (dict(radius=5), "radius"), (dict(tile=-1), "tile"), (dict(tile=3), "tile"),
            (dict(gate_bits=nan32), "gate"), (dict(gate_bits=neg32), "gate"),
            (dict(inv_bin_bits=nan32), "inv_bin"), (dict(inv_bin_bits=inf32), "inv_bin"), (dict(inv_bin_bits=0), "inv_bin"),
            (dict(inv_bin_bits=neg32), "inv_bin"),
            (dict(depth=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(wr=None), "null pointer"),
            (dict(H=16 * 65535 + 1, W=8, levels=1, tile=2), "rows of tiles")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err and "ud_depth_pyramid" in err, (kw, rc, err)
    # (nothing else can be called here: a descriptor that passes every check would be launched)


# ---- argument checks, no GPU -----------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    from unidepth_amd import pyramid
    d = torch.ones(2, 1, 9, 12)
    for fn in (pyramid.depth_pyramid, pyramid.depth_pyramid_composition):
        name = fn.__name__
        for args, kw, msg in (
                ((torch.ones(2, 9, 12, dtype=torch.int32),), {}, "float tensor"), ((torch.ones(2, 2, 9, 12),), {}, r"\[B,1,H,W\]"),
                ((torch.ones(0, 1, 9, 12),), {}, "non-empty"), ((torch.ones(257, 1, 4, 4),), {}, "at most 256"),
                ((d, 0), {}, "levels"), ((d, 5), {}, "levels"), ((d, True), {}, "levels"), ((d, 2.0), {}, "levels"), ((torch.ones(2, 1, 7, 12), 4), {}, "need H, W >= 8"),
                ((d,), dict(mask=torch.ones(2, 1, 9, 12)), "bool or uint8"), ((d,), dict(mask=torch.ones(2, 1, 9, 11, dtype=torch.bool)), "mask"),
                ((d,), dict(mask=torch.ones(1, 1, 9, 12, dtype=torch.bool)), "mask of 1 images"),
                ((d,), dict(weights=torch.ones(2, 1, 9, 12, dtype=torch.uint8)), "float tensor"), ((d,), dict(weights=torch.ones(2, 1, 8, 12)), "weights"),
                ((d,), dict(filter=(1, 2)), "prepare_depth_filter"), ((d,), dict(gate=-1.0), "gate"), ((d,), dict(gate=float("nan")), "gate"),
                ((d,), dict(gate="x"), "gate"), ((d,), dict(gate=True), "gate")):
            with pytest.raises(ValueError, match=f"{name}: .*{msg}"):
                fn(*args, **kw)
        with pytest.raises(RuntimeError, match=f"{name}: GPU tensors"):
            fn(d)
    for args, msg in (((5, 1.0, 0.1), "radius"), ((-1, 1.0, 0.1), "radius"), ((True, 1.0, 0.1), "radius"), ((1.5, 1.0, 0.1), "radius"),
                      ((1, 0.0, 0.1), "sigma_space"), ((1, float("inf"), 0.1), "sigma_space"), ((1, "a", 0.1), "sigma_space"),
                      ((1, 1.0, -0.1), "sigma_range"), ((1, 1.0, float("nan")), "sigma_range")):
        with pytest.raises(ValueError, match=f"prepare_depth_filter: .*{msg}"):
            pyramid.prepare_depth_filter(*args, "cpu")
    with pytest.raises(RuntimeError, match="prepare_depth_filter: GPU tensors"):
        pyramid.prepare_depth_filter(1, 1.0, 0.1, "cpu")
    K = torch.tensor([[50.0, 0, 6], [0, 50.0, 4.5], [0, 0, 1]])
    for levels in (0, 5, True, 1.0):
        with pytest.raises(ValueError, match="pyramid_cameras: levels"):
            pyramid.pyramid_cameras(K, 2, levels, "cpu")
    with pytest.raises(RuntimeError, match="GPU tensors"):
        pyramid.pyramid_cameras(K, 2, 2, "cpu")
    m = (torch.ones(2, 3, 9, 12), torch.ones(2, 3, 9, 12), torch.ones(2, 1, 9, 12, dtype=torch.bool), K)
    track = pyramid.track_camera_pyramid
    for args, kw, msg in (
            ((torch.ones(2, 3, 9, 12), K, [m]), {}, "point map"), ((d, K, 5), {}, "model_levels"), ((d, K, []), {}, "model_levels"),
            ((d, K, [m] * 5), {}, "model_levels"), ((d, K, [m[:3]]), {}, "model_levels"),
            ((d, K, [m, m]), dict(iters=(3,)), "iters"), ((d, K, [m, m]), dict(iters=(0, 0)), "iters"), ((d, K, [m, m]), dict(iters=(1, -1)), "iters"),
            ((d, K, [m, m]), dict(iters=(1, 2.0)), "iters"), ((d, K, [m, m]), dict(iters=4), "iters"), ((d, K, [m, m]), dict(iters=(1, 1001)), "iters"),
            ((d, K, [m]), dict(iters=(2,), damping=-1.0), "damping"), ((d, K, [m]), dict(iters=(2,), min_count=-1), "min_count"),
            ((torch.ones(2, 1, 7, 12), K, [m] * 4), dict(iters=(1, 1, 1, 1)), "need H, W >= 8"), ((d, K, [m]), dict(iters=(1,), gate=-2), "gate")):
        with pytest.raises(ValueError, match=f"track_camera_pyramid: .*{msg}"):
            track(*args, dist_tol=0.1, **kw)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        track(d, K, [m], iters=(2,), dist_tol=0.1)
    assert math.isinf(float(np.array([pc.INF_BITS], np.int32).view(F)[0]))
