"""tsdf_integrate / tsdf_points without a GPU (unidepth_amd/tsdf.py, include/unidepth_hip.h UdTsdfIntegrate / UdTsdfPoints): the fused
per-voxel function of csrc/tsdf_point.h compiled for the host and run under the host sanitizers (tests/tsdf_host/tsdf_host.cpp, a
stand-alone program) against the chain of the unchanged per-point functions with every intermediate in memory, bit for bit, for all six
view models, shared and per-image transforms and origins, every optional input, a fresh and a continued volume; ud_tsdf_slot against its
numpy restatement; the known answer and the special values; the C-ABI's descriptors, every refusal of both entry points and the Python
argument errors.  Shared helpers: tests/tsdf_common.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import tsdf_common as tc

ROOT = tc.ROOT
SETS = {**{tc.NAMES[m]: m for m in tc.MODELS}, "mixed": tc.mixed_models()}
OPTIONS = (dict(src_masks=True), dict(src_weights=True), dict(images=True), dict(max_weight=tc.MAX_WEIGHT))
ALL = dict(src_masks=True, src_weights=True, images=True, max_weight=tc.MAX_WEIGHT)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return tc.build_host(tmp_path_factory)


def _same(a, b, names=("tsdf", "weight", "color", "count")):
    return all((a[k] is None and b[k] is None) or tc.host_program.same_bits(a[k], b[k]) for k in names)


def _check_slots(r, s):
    """the program's ud_tsdf_slot results against the numpy restatement, bit for bit"""
    live, xyz, rgb = tc.slots(r["tsdf"], r["weight"], r["color"], s["origin"], s["voxel"], r["min_weight"])
    assert np.array_equal(live, r["live"])
    assert tc.host_program.same_bits(xyz, r["xyz"])
    if rgb is not None:
        assert tc.host_program.same_bits(rgb, r["rgb_f32"]) and np.array_equal(tc.to_u8(rgb), r["rgb_u8"])


# ---- the fused function against the chain, on the host --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SETS))
def test_host_fused_equals_chain_for_every_model(host, name):
    """each of the six models as the view model of every view, and one batch that mixes all six: B = 2, V = 3 on the base scene, shared and
    per-image transforms and origins, each optional input on and off, a fresh and a continued volume.  The program exits non-zero when
    the fused function and the chain differ in one bit or a sanitizer reports.  No comparison is vacuous (tsdf_common.assert_not_vacuous)
    and every optional input changes at least one output bit."""
    for per in (False, True):
        s = tc.scene(SETS[name], per_image=per, per_origin=per, **tc.BASE)
        if name == "mixed":
            assert {m for row in s["models"] for m in row} == set(tc.MODELS)
        plain = tc.host_tsdf(host, s)
        tc.assert_not_vacuous(name, plain, tc.view_counts(host, s))
        _check_slots(plain, s)
        assert plain["color"] is None and np.array_equal(plain["weight"], plain["count"].astype(np.float32))
        for opt in OPTIONS:
            r = tc.host_tsdf(host, s, **opt)
            if "images" in opt:                                                 # colours change nothing else
                assert _same(r, plain, ("tsdf", "weight", "count")) and r["color"].any()
            else:
                assert not _same(r, plain, ("tsdf", "weight", "count")), (name, per, opt)
        full = tc.host_tsdf(host, s, min_weight=0.75, **ALL)
        tc.assert_not_vacuous(name, full, tc.view_counts(host, s, **ALL))
        _check_slots(full, s)
        assert full["live"].any() and (full["rgb_u8"][full["live"]] > 0).any()
        # a continued volume: the first view, then the other two, has the bits of one call over all three
        for kw in (ALL, dict(src_weights=True, images=True)):
            first = tc.host_tsdf(host, s, views=slice(0, 1), **kw)
            rest = tc.host_tsdf(host, s, views=slice(1, 3), volume=(first["tsdf"], first["weight"], first["color"]), **kw)
            whole = full if kw is ALL else tc.host_tsdf(host, s, **kw)
            assert _same(rest, whole, ("tsdf", "weight", "color"))
            assert np.array_equal(first["count"] + rest["count"], whole["count"])


def test_host_second_scene(host):
    s = tc.scene(tc.mixed_models(), per_image=True, **tc.SECOND)
    for kw in ({}, ALL):
        r = tc.host_tsdf(host, s, **kw)
        tc.assert_not_vacuous("second", r, tc.view_counts(host, s, **kw))
        _check_slots(r, s)


@pytest.mark.parametrize("name", list(tc.EDGES))
def test_host_edge_scenes(host, name):
    """the scenes of the GPU edge tests, through the host program: fused equals chain, the sanitizers are silent, the slots equal their
    restatement, and no scene is vacuous"""
    s = tc.scene(**tc.EDGES[name])
    for kw in ({}, ALL):
        r = tc.host_tsdf(host, s, min_weight=0.5, **kw)
        tc.assert_not_vacuous(name, r, tc.view_counts(host, s, **kw))
        _check_slots(r, s)


def test_host_known_answer(host):
    s = tc.known_answer_scene()
    r = tc.host_tsdf(host, s)
    tc.check_known_answer(r["tsdf"], r["weight"], r["count"], r["live"], r["xyz"])
    _check_slots(r, s)


@pytest.mark.parametrize("weights", (False, True))
def test_host_special_values(host, weights):
    """NaN, +-inf, 0, -0.0 and negatives in the depths; NaN, 0, inf and negatives in the weights; voxels behind every view; a singular
    Pinhole row: the program's own comparison with the chain (and the sanitizers), and no voxel is updated that its inputs cannot support"""
    s = tc.special_scene()
    for masks in (False, True):
        r = tc.host_tsdf(host, s, src_masks=masks, src_weights=weights, images=True, min_weight=0.5)
        tc.check_special(r, s, weights)
        _check_slots(r, s)
    with_nan = np.array(r["tsdf"])
    with_nan[0, 4] = np.nan                                                       # a NaN distance is no crossing
    live, _, _ = tc.slots(with_nan, r["weight"], None, s["origin"], s["voxel"], 0.5)
    assert live.sum() < r["live"].sum()


def test_slot_restatement_on_a_planted_volume():
    """the restatement itself, on a volume whose answer is known by hand: one crossing along +x at t = 0.25, its weights gate it"""
    tsdf = np.ones((1, 1, 1, 3), np.float32)
    tsdf[0, 0, 0] = [0.25, -0.75, -1.0]
    w = np.array([2.0, 1.0, 0.5], np.float32).reshape(1, 1, 1, 3)
    col = np.zeros((1, 3, 1, 1, 3), np.float32)
    col[0, 0, 0, 0] = [100.0, 102.0, 7.0]
    live, xyz, rgb = tc.slots(tsdf, w, col, np.zeros((1, 3), np.float32), 0.5, 1.0)
    assert live.tolist() == [[True] + [False] * 8]
    assert xyz[0, 0].tolist() == [0.25 + 0.25 * 0.5, 0.25, 0.25] and rgb[0, 0].tolist() == [100.5, 0.0, 0.0]
    assert tc.to_u8(rgb[0, 0]).tolist() == [100, 0, 0] and tc.to_u8(np.array([101.5, -3.0, 300.0, np.nan], np.float32)).tolist() == [102, 0, 255, 0]
    assert not tc.slots(tsdf, w, None, np.zeros((1, 3), np.float32), 0.5, 1.5)[0].any()


def test_many_tiles_volumes_reach_the_second_chunk_of_the_scan():
    """the input of test_tsdf_gpu's 257-tile case: live slots in the tiles 0, 255 and 256 of both volumes (its own assertions)"""
    (t, w, c, o), voxel = tc.many_tiles_volumes()
    assert t.shape == (2, 16, 8, 683) and c.shape == (2, 3, 16, 8, 683) and not np.array_equal(t[0], t[1])


def test_points_capacity_and_workspace_errors_without_gpu():
    """tsdf_points' share of the packing tail it has in common with pack_points (pointcloud._packed): refused in its own sentences
    before anything is allocated or run (a volume itself must live on the GPU: tests/test_tsdf_gpu.py test_python_surface)"""
    from unidepth_amd.pointcloud import _packed
    cpu = torch.device("cpu")
    odd = torch.empty(1 << 10, dtype=torch.uint8)[1:]
    assert odd.data_ptr() % 8
    for kw, what in ((dict(capacity=True), "capacity"), (dict(capacity=-1), "capacity"), (dict(capacity=1.5), "capacity"),
                     (dict(workspace=bytearray(1 << 10)), "workspace"), (dict(workspace=odd), "workspace"),
                     (dict(workspace=torch.empty(8, dtype=torch.uint8)), "workspace"), (dict(workspace=torch.empty(1 << 10)), "workspace"),
                     (dict(workspace=torch.empty(1 << 10, dtype=torch.uint8)[::2]), "workspace")):
        with pytest.raises(ValueError, match=f"tsdf_points: {what} must be"):
            _packed("tsdf_points", cpu, 2, 136, None, kw.get("capacity"), kw.get("workspace"), torch.uint8, False)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_tsdf_points_workspace_size():
    """16 ballot words and two int32 per tile of 1024 slots, -1 outside the limits"""
    from unidepth_amd import _lib
    wb = _lib.lib.ud_tsdf_points_work_bytes
    assert wb(1, 341, 1, 1) == 136 and wb(1, 342, 1, 1) == 272 and wb(3, 683, 1, 1) == 3 * 3 * 136
    assert wb(0, 1, 1, 1) == -1 and wb(1, 0, 1, 1) == -1 and wb(1, 1024, 1024, 683) == -1 and wb(65536, 1, 1, 1) == -1


def test_every_refusal_of_integrate():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_tsdf_integrate(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    nan, inf, neg, zero = (tc.f32_bits(v) for v in (float("nan"), float("inf"), -0.5, 0.0))

    def call(**kw):
        d = _lib.UdTsdfIntegrate()
        base = dict(src_depth=16, src_mask=None, src_weight=None, image=None, params=16, T=16, origin=16, tsdf=16, weight=16, color=None,
                    count=None, B=2, V=3, Nx=4, Ny=5, Nz=6, Hs=5, Ws=7, nT=1, n_origin=1, fresh=1, has_max_weight=0,
                    voxel_size_bits=tc.f32_bits(0.1), trunc_bits=tc.f32_bits(0.3), max_weight_bits=0)
        base.update(kw)
        models = base.pop("models", (1, 2, 3, 4, 5, 6))
        for k, v in base.items():
            setattr(d, k, v)
        for k, m in enumerate(models):
            d.model[k] = m
        return lib.ud_tsdf_integrate(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in (
            (dict(B=0), "bad sizes"), (dict(V=0), "bad sizes"), (dict(B=-1), "bad sizes"), (dict(B=1, V=256), "bad sizes"), (dict(B=2, V=129), "bad sizes"),
            (dict(B=257, V=1), "bad sizes"), (dict(B=65536, V=65536), "bad sizes"), (dict(Nx=0), "bad sizes"), (dict(Ny=-1), "bad sizes"),
            (dict(Nz=0), "bad sizes"), (dict(Hs=0), "bad sizes"), (dict(Ws=-2), "bad sizes"),
            (dict(Nx=1 << 11, Ny=1 << 10, Nz=1 << 10), "too large"), (dict(Nx=2 ** 31 - 1, Ny=2 ** 31 - 1, Nz=1), "too large"),
            (dict(Nx=2 ** 31 - 256, Ny=1, Nz=1), "too large"), (dict(Nx=1 << 16, Ny=1 << 16, Nz=1 << 16), "too large"),
            (dict(Hs=1 << 16, Ws=1 << 15), "too large"), (dict(Hs=1 << 14, Ws=1 << 14), "too large"), (dict(Hs=2 ** 31 - 1, Ws=2 ** 31 - 1), "too large"),
            (dict(src_depth=None), "null pointer"), (dict(params=None), "null pointer"), (dict(T=None), "null pointer"),
            (dict(origin=None), "null pointer"), (dict(tsdf=None), "null pointer"), (dict(weight=None), "null pointer"),
            (dict(image=16), "image and color"), (dict(color=16), "image and color"),
            (dict(nT=0), "nT"), (dict(nT=3), "nT"), (dict(n_origin=0), "n_origin"), (dict(n_origin=3), "n_origin"),
            (dict(voxel_size_bits=nan), "voxel_size"), (dict(voxel_size_bits=inf), "voxel_size"), (dict(voxel_size_bits=neg), "voxel_size"),
            (dict(voxel_size_bits=zero), "voxel_size"), (dict(trunc_bits=nan), "trunc"), (dict(trunc_bits=inf), "trunc"),
            (dict(trunc_bits=neg), "trunc"), (dict(trunc_bits=zero), "trunc"),
            (dict(has_max_weight=1, max_weight_bits=nan), "max_weight"), (dict(has_max_weight=1, max_weight_bits=inf), "max_weight"),
            (dict(has_max_weight=1, max_weight_bits=neg), "max_weight"), (dict(has_max_weight=1, max_weight_bits=zero), "max_weight"),
            (dict(models=(1, 2, 3, 4, 5, 0)), "model tag"), (dict(models=(7, 2, 3, 4, 5, 6)), "model tag")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err and err.startswith("ud_tsdf_integrate: "), (kw, rc, err)
    # (nothing else can be called here: a descriptor that passes every check would be launched)


def test_every_refusal_of_points():
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_tsdf_points(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    need = lib.ud_tsdf_points_work_bytes(2, 4, 5, 6)

    def call(**kw):
        d = _lib.UdTsdfPoints()
        base = dict(tsdf=16, weight=16, color=None, origin=16, xyz=16, rgb=None, counts=16, offsets=16, work=16, work_bytes=need, capacity=10,
                    B=2, Nx=4, Ny=5, Nz=6, n_origin=1, rgb_f32=0, voxel_size_bits=tc.f32_bits(0.1), min_weight_bits=tc.f32_bits(1.0))
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.ud_tsdf_points(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in (
            (dict(B=0), "bad sizes"), (dict(B=65536), "bad sizes"), (dict(Nx=0), "bad sizes"), (dict(Ny=-1), "bad sizes"), (dict(Nz=0), "bad sizes"),
            (dict(capacity=-1), "bad sizes"), (dict(Nx=1 << 10, Ny=1 << 10, Nz=683), "bad sizes"), (dict(Nx=2 ** 31 - 1, Ny=2 ** 31 - 1, Nz=2), "bad sizes"),
            (dict(tsdf=None), "null pointer"), (dict(weight=None), "null pointer"), (dict(origin=None), "null pointer"),
            (dict(counts=None), "null pointer"), (dict(offsets=None), "null pointer"), (dict(work=None), "null pointer"), (dict(work=20), "null pointer"),
            (dict(rgb=16), "rgb needs"), (dict(rgb=16, color=16, xyz=None), "rgb needs"),
            (dict(n_origin=0), "n_origin"), (dict(n_origin=3), "n_origin"),
            (dict(voxel_size_bits=tc.f32_bits(float("nan"))), "voxel_size"), (dict(voxel_size_bits=tc.f32_bits(float("inf"))), "voxel_size"),
            (dict(voxel_size_bits=tc.f32_bits(0.0)), "voxel_size"), (dict(voxel_size_bits=tc.f32_bits(-1.0)), "voxel_size"),
            (dict(min_weight_bits=tc.f32_bits(float("nan"))), "min_weight"),
            (dict(work_bytes=need - 1), "workspace smaller"), (dict(work_bytes=0), "workspace smaller")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err and err.startswith("ud_tsdf_points: "), (kw, rc, err)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, tsdf
    K = torch.tensor([[9.0, 0, 9.5], [0, 9.0, 5.5], [0, 0, 1]])
    depths, T = torch.rand(2, 3, 5, 7) + 1, torch.eye(4).repeat(3, 1, 1)
    cams = [K, K, K]
    fresh = dict(grid_shape=(3, 4, 5), origin=(0.0, 0.0, 1.0), voxel_size=0.1, trunc=0.3)
    for f in (tsdf.tsdf_integrate, tsdf.tsdf_integrate_composition):
        fn = f.__name__

        def bad(match, *args, exc=ValueError, **kw):
            with pytest.raises(exc, match=match):
                f(None, *args, **{**fresh, **kw})
        for d in (torch.rand(2, 5, 7), torch.ones(2, 3, 5, 7, dtype=torch.int32), torch.rand(2, 0, 5, 7), "depths"):
            bad(f"{fn}: depths", d, cams, T)
        bad(f"{fn}: depths: at most", torch.rand(2, 129, 1, 1), [K] * 129, torch.eye(4).repeat(129, 1, 1))
        bad(f"{fn}: depths: at most", torch.rand(1, 256, 1, 1), [K] * 256, torch.eye(4).repeat(256, 1, 1))
        for c in ([K, K], K, (K,) * 4, None):
            bad(f"{fn}: cameras", depths, c, T)
        bad(fn + r": cameras\[1\] of 3 images", depths, [K, cameras.BatchCamera([cameras.Pinhole(K)] * 3), K], T)
        for t in (torch.eye(4), torch.eye(4).repeat(2, 1, 1), T.double(), torch.rand(3, 3, 3), torch.rand(3, 3, 4, 4), None):
            bad(f"{fn}: transforms", depths, cams, t)
        for name in ("trunc", "voxel_size", "max_weight"):
            for v in (0, -0.1, float("nan"), float("inf"), 1e300, "x", True) + ((None,) if name != "max_weight" else ()):
                bad(f"{fn}: {name}", depths, cams, T, **{name: v})
        for g in ((3, 4), (0, 4, 5), 7, None, ("a", 1, 2)):
            bad(f"{fn}: grid_shape", depths, cams, T, grid_shape=g)
        for o in ((0.0, 1.0), torch.zeros(3, dtype=torch.float64), torch.zeros(3, 3), None, "abc"):
            bad(f"{fn}: origin", depths, cams, T, origin=o)
        for m in (torch.ones(2, 3, 5, 6, dtype=torch.bool), torch.ones(2, 3, 5, 7), torch.ones(2, 1, 5, 7, dtype=torch.bool), "m"):
            bad(f"{fn}: src_masks", depths, cams, T, src_masks=m)
        for w in (torch.ones(2, 3, 5, 6), torch.ones(2, 3, 5, 7, dtype=torch.uint8), "w"):
            bad(f"{fn}: src_weights", depths, cams, T, src_weights=w)
        for im in (torch.zeros(2, 3, 3, 5, 6, dtype=torch.uint8), torch.zeros(2, 3, 3, 5, 7), torch.zeros(2, 3, 5, 7, dtype=torch.uint8), "i"):
            bad(f"{fn}: images", depths, cams, T, images=im)
        bad(f"{fn}: unsupported sizes", depths, cams, T, grid_shape=(1 << 11, 1 << 10, 1 << 10))
        # a given volume: a TsdfVolume of contiguous fp32 GPU tensors, which carries its own grid
        cpu_volume = tsdf.TsdfVolume(torch.ones(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), None, torch.zeros(1, 3), 0.1)
        with pytest.raises(ValueError, match=f"{fn}: volume.tsdf must be a contiguous fp32 GPU tensor"):
            f(cpu_volume, depths, cams, T, trunc=0.3)
        with pytest.raises(ValueError, match=f"{fn}: volume must be a TsdfVolume"):
            f((1, 2), depths, cams, T, trunc=0.3)
        with pytest.raises(ValueError, match=f"{fn}: grid_shape, origin and voxel_size describe a fresh volume"):
            f(cpu_volume, depths, cams, T, trunc=0.3, voxel_size=0.1)
        with pytest.raises(NotImplementedError):
            f(None, depths, [K, object(), K], T, **fresh)
        # well-formed arguments on the CPU: the HIP kernels are the only implementation
        eucm = cameras.EUCM(torch.tensor([9.0, 9, 9.5, 5.5, 0.5, 1.0]))
        opencv = cameras.OPENCV(torch.tensor([9.0, 9, 9.5, 5.5] + [0.0] * 12))
        for args, kw in (((depths, cams, T), {}), ((depths.double(), (K, opencv, eucm), T[:, :3]), dict(max_weight=2, return_count=True)),
                         ((depths, cams, torch.eye(4)[:3].repeat(2, 3, 1, 1)),
                          dict(src_masks=torch.ones(2, 3, 5, 7, dtype=torch.bool), src_weights=torch.ones(2, 3, 5, 7, dtype=torch.float64),
                               images=torch.zeros(2, 3, 3, 5, 7, dtype=torch.uint8), origin=torch.zeros(2, 3)))):
            bad("GPU", *args, exc=RuntimeError, **kw)
    cpu_volume = tsdf.TsdfVolume(torch.ones(2, 3, 4, 5), torch.zeros(2, 3, 4, 5), None, torch.zeros(1, 3), 0.1)
    with pytest.raises(ValueError, match="tsdf_points: volume.tsdf must be a contiguous fp32 GPU tensor"):
        tsdf.tsdf_points(cpu_volume)
    with pytest.raises(ValueError, match="tsdf_points: volume must be a TsdfVolume"):
        tsdf.tsdf_points(torch.ones(2, 3, 4, 5))
    for name in ("TsdfVolume", "tsdf_integrate", "tsdf_integrate_composition", "tsdf_points"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(tsdf, name)
    doc = tsdf.tsdf_integrate.__doc__
    assert "repeated calls" in doc and "PreparedCamera" in doc and "All six camera models" in doc
