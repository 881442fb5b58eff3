"""depth_consistency without a GPU (unidepth_amd/consistency.py, include/unidepth_hip.h UdDepthConsistency): the fused per-pixel function
of csrc/consistency_point.h compiled for the host and run under the host sanitizers (tests/consistency_host/consistency_host.cpp, a
stand-alone program) against the chain of the unchanged per-point functions with every intermediate in memory, bit for bit, for every
(reference, view) pair of the four closed-form models, shared and per-image transforms, with and without src_masks and valid_in, on the
known answer and on the special values; the C-ABI's descriptor, every refusal of the entry point, the Python argument errors and
invert_rigid.  Shared helpers: tests/consistency_common.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import consistency_common as cc

ROOT = cc.ROOT
REF_SETS = {"pinhole": (cc.PINHOLE,) * 4, "eucm": (cc.EUCM,) * 4, "spherical": (cc.SPHERICAL,) * 4, "mei": (cc.MEI,) * 4,
            "mixed": (cc.MEI, cc.SPHERICAL, cc.EUCM, cc.PINHOLE)}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cc.build_host(tmp_path_factory)


# ---- the fused function against the chain, on the host --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(REF_SETS))
def test_host_fused_equals_chain_for_every_model_pair(host, name):
    """each closed-form reference model against views of all four (every image of the batch of four meets three of them, every view holds
    all four), reference 13x17, views 11x19, V = 3; shared and per-image transforms; with and without src_masks and valid_in; min_views 0,
    1 and V.  The program exits non-zero when the fused function and the chain differ in one bit or a sanitizer reports.  Every view's
    consistent share lies strictly between 10 % and 90 %, in every run."""
    pairs = set()
    for per_image in (False, True):
        s = cc.scene(REF_SETS[name], per_image=per_image)
        pairs |= {(s["models_ref"][b], s["models_src"][v][b]) for v in range(s["V"]) for b in range(s["B"])}
        plain = None
        for masks, vin, min_views in ((False, False, 1), (True, True, 0), (True, False, 3), (False, True, 1)):
            r = cc.host_scene(host, s, min_views=min_views, valid_in=s["valid_in"] if vin else None, src_masks=s["src_masks"] if masks else None)
            cc.assert_shares(r["consistent"], (name, per_image, masks, vin))
            d = s["depth"][:, 0]
            ref_ok = (d > 0) & ((s["valid_in"] != 0) if vin else True)
            assert (~ref_ok).mean() > (0.08 if vin else 0.03)
            assert (r["fused"][~ref_ok] == 0).all() and not r["count"][~ref_ok].any() and not r["mask"][~ref_ok].any()
            assert np.array_equal(r["count"], r["consistent"].sum(axis=1).astype(np.uint8))
            assert np.array_equal(r["mask"], ref_ok & (r["count"] >= min_views))
            live = ref_ok & (r["count"] > 0)
            assert (np.abs(r["fused"][live] / d[live] - 1) <= cc.REL_TOL * 1.0001).all()            # a mean of values within rel_tol of depth
            assert (r["err_px"][r["consistent"]] <= cc.PX_TOL).all() and (r["err_rel"][r["consistent"]] <= cc.REL_TOL * 1.0001).all()
            if plain is None:
                plain = r
            else:                                                                                  # the optional inputs are read
                assert not np.array_equal(r["consistent"], plain["consistent"])
    if name != "mixed":
        assert pairs == {(REF_SETS[name][0], m) for m in cc.CLOSED}


@pytest.mark.parametrize("name", list(cc.EDGES))
def test_host_edge_scenes(host, name):
    """the scenes of the GPU edge tests, through the host program: fused equals chain, the sanitizers are silent, and no scene is vacuous"""
    kw, call = cc.EDGES[name]
    s = cc.scene(**kw)
    r = cc.host_scene(host, s, valid_in=s["valid_in"], src_masks=s["src_masks"], **call)
    cc.assert_edge_shares(name, r["consistent"])


@pytest.mark.parametrize("ref", cc.CLOSED)
def test_host_gpu_matrix_scenes_are_not_vacuous(host, ref):
    """the 37x53 <- 29x41 scenes the GPU matrix runs (B = 3 with V = 3, shared and per-image; B = 1 with four views of four models)"""
    for kw in (dict(ref_models=(ref,) * 3, per_image=False), dict(ref_models=(ref,) * 3, per_image=True), dict(ref_models=(ref,), V=4)):
        s = cc.scene(**kw, **cc.BIG)
        assert {m for row in s["models_src"] for m in row} == set(cc.CLOSED)
        for opt in (False, True):
            r = cc.host_scene(host, s, valid_in=s["valid_in"] if opt else None, src_masks=s["src_masks"] if opt else None)
            cc.assert_shares(r["consistent"], (ref, kw, opt))


def test_host_tolerances_decide(host):
    """the off-plane blocks (10 % off) are what a rel_tol of 1 % rejects: a rel_tol of 20 % accepts most of them; a px_tol of 0 accepts
    next to nothing"""
    s = cc.scene(REF_SETS["mixed"])
    tight, loose, zero = (cc.host_scene(host, s, **kw)["consistent"].mean() for kw in (dict(), dict(rel_tol=0.2, px_tol=2.0), dict(px_tol=0.0)))
    assert loose > tight + 0.15 and zero < 0.02, (tight, loose, zero)


def test_host_known_answer(host):
    k = cc.known_answer_inputs()

    def run(depth, rel_tol):
        return cc.host_consistency(host, depth, k["rows"], k["models"], k["src_depths"], k["rows_src"], k["models_src"], k["T"], rel_tol=rel_tol)
    cc.check_known_answer(run)


@pytest.mark.parametrize("min_views", (0, 1))
def test_host_special_values(host, min_views):
    """NaN, +-inf, 0, -0.0 and negative values in depth and src_depths, a singular Pinhole row on either side, points behind every view:
    the program's own comparison with the chain (and the sanitizers), and no decision is true of a pixel whose inputs cannot support it"""
    s = cc.special_case()
    for masks in (False, True):
        r = cc.host_scene(host, s, min_views=min_views, src_masks=s["src_masks"] if masks else None)
        cc.check_special(r, s, min_views)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_consistency_descriptor_ends_with_the_model_arrays_and_has_no_float_field():
    from unidepth_amd import _lib
    fields = _lib.UdDepthConsistency._fields_
    assert [n for n, _ in fields[-2:]] == ["model_ref", "model_src"]
    assert all(t in (C.c_void_p, C.c_int) for _, t in fields[:-2])


def test_every_refusal():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_depth_consistency(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    nan_bits, inf_bits, neg_bits = cc.f32_bits(float("nan")), cc.f32_bits(float("inf")), cc.f32_bits(-0.5)

    def call(**kw):
        d = _lib.UdDepthConsistency()
        base = dict(depth=16, params_ref=16, valid_in=None, src_depth=16, src_mask=None, params_src=16, T=16, Tinv=16, fused=16, count=16,
                    mask=16, consistent=None, err_px=None, err_rel=None, B=2, V=3, H=4, W=6, Hs=5, Ws=7, nT=1, min_views=1,
                    px_tol_bits=cc.f32_bits(1.0), rel_tol_bits=cc.f32_bits(0.01))
        base.update(kw)
        ref, views = base.pop("ref", (1, 6)), base.pop("views", (1, 2, 3, 6, 2, 1) + (1,) * 250)
        for k, v in base.items():
            setattr(d, k, v)
        for b, m in enumerate(ref):
            d.model_ref[b] = m
        for k, m in enumerate(views):
            d.model_src[k] = m
        return lib.ud_depth_consistency(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg, rc_want in (
            (dict(B=0), "bad sizes", -1), (dict(V=0), "bad sizes", -1), (dict(B=-1), "bad sizes", -1), (dict(B=1, V=256), "bad sizes", -1),
            (dict(B=2, V=129), "bad sizes", -1), (dict(B=257, V=1), "bad sizes", -1), (dict(B=65536, V=65536), "bad sizes", -1),
            (dict(H=0), "bad sizes", -1), (dict(W=-1), "bad sizes", -1), (dict(Hs=0), "bad sizes", -1), (dict(Ws=-2), "bad sizes", -1),
            (dict(H=1 << 16, W=1 << 15), "too large", -1), (dict(H=1, W=2 ** 31 - 256), "too large", -1), (dict(Hs=1 << 16, Ws=1 << 15), "too large", -1),
            (dict(Hs=1 << 15, Ws=1 << 15), "too large", -1), (dict(Hs=2 ** 31 - 1, Ws=2 ** 31 - 1), "too large", -1),
            (dict(depth=None), "null pointer", -1), (dict(params_ref=None), "null pointer", -1), (dict(src_depth=None), "null pointer", -1),
            (dict(params_src=None), "null pointer", -1), (dict(T=None), "null pointer", -1), (dict(Tinv=None), "null pointer", -1),
            (dict(fused=None), "null pointer", -1), (dict(count=None), "null pointer", -1), (dict(mask=None), "null pointer", -1),
            (dict(nT=0), "nT", -1), (dict(nT=3), "nT", -1),
            (dict(px_tol_bits=nan_bits), "px_tol", -1), (dict(px_tol_bits=inf_bits), "px_tol", -1), (dict(px_tol_bits=neg_bits), "px_tol", -1),
            (dict(rel_tol_bits=nan_bits), "rel_tol", -1), (dict(rel_tol_bits=inf_bits), "rel_tol", -1), (dict(rel_tol_bits=neg_bits), "rel_tol", -1),
            (dict(min_views=-1), "min_views", -1), (dict(min_views=4), "min_views", -1),
            (dict(ref=(0, 1)), "model tag", -1), (dict(ref=(1, 7)), "model tag", -1), (dict(views=(1, 2, 3, 6, 2, 0)), "model tag", -1),
            (dict(views=(9, 2, 3, 6, 2, 1)), "model tag", -1),
            (dict(ref=(4, 1)), "iterative model", -3), (dict(ref=(1, 5)), "iterative model", -3), (dict(views=(1, 2, 3, 6, 2, 4)), "iterative model", -3),
            (dict(views=(5, 2, 3, 6, 2, 1)), "iterative model", -3)):
        rc, err = call(**kw)
        assert rc == rc_want and msg in err, (kw, rc, err)
    # (nothing else can be called here: a descriptor that passes every check would be launched)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, consistency
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    depth, src, T = torch.rand(2, 1, 4, 6) + 1, torch.rand(2, 3, 5, 7) + 1, torch.eye(4).repeat(3, 1, 1)
    cams = [K, K, K]
    for f in (consistency.depth_consistency, consistency.depth_consistency_composition):
        fn = f.__name__
        for bad in (torch.rand(2, 2, 4, 6), torch.rand(4, 6), torch.ones(2, 1, 4, 6, dtype=torch.int64), torch.rand(0, 1, 4, 6), "depth"):
            with pytest.raises(ValueError, match=f"{fn}: depth"):
                f(bad, K, src, cams, T)
        for bad in (torch.rand(3, 3, 5, 7), torch.rand(2, 5, 7), torch.ones(2, 3, 5, 7, dtype=torch.int32), torch.rand(2, 0, 5, 7), "src"):
            with pytest.raises(ValueError, match=f"{fn}: src_depths"):
                f(depth, K, bad, cams, T)
        with pytest.raises(ValueError, match=f"{fn}: src_depths: at most"):
            f(depth, K, torch.rand(2, 129, 1, 1), [K] * 129, torch.eye(4).repeat(129, 1, 1))
        with pytest.raises(ValueError, match=f"{fn}: src_depths: at most"):
            f(depth[:1], K, torch.rand(1, 256, 1, 1), [K] * 256, torch.eye(4).repeat(256, 1, 1))
        for bad in ([K, K], K, (K,) * 4, None):
            with pytest.raises(ValueError, match=f"{fn}: src_cameras"):
                f(depth, K, src, bad, T)
        with pytest.raises(ValueError, match=f"{fn}: camera of 3 images"):
            f(depth, K.expand(3, 3, 3), src, cams, T)
        with pytest.raises(ValueError, match=fn + r": src_cameras\[1\] of 3 images"):
            f(depth, K, src, [K, cameras.BatchCamera([cameras.Pinhole(K)] * 3), K], T)
        for bad in (torch.eye(4), torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(3, 1, 1).double(), torch.rand(3, 3, 3), torch.rand(3, 3, 4, 4),
                    torch.rand(3, 2, 3, 4), None):
            with pytest.raises(ValueError, match=f"{fn}: transforms"):
                f(depth, K, src, cams, bad)
        for name in ("px_tol", "rel_tol"):
            for bad in (-0.1, float("nan"), float("inf"), 1e300, "tol", None):
                with pytest.raises(ValueError, match=f"{fn}: {name}"):
                    f(depth, K, src, cams, T, **{name: bad})
        for bad in (-1, 4, 1.0, True, None):
            with pytest.raises(ValueError, match=f"{fn}: min_views"):
                f(depth, K, src, cams, T, min_views=bad)
        for bad in (torch.ones(2, 1, 4, 5, dtype=torch.bool), torch.ones(2, 4, 6), torch.ones(1, 4, 6, dtype=torch.bool), torch.ones(2, 24, dtype=torch.bool), "m"):
            with pytest.raises(ValueError, match=f"{fn}: valid_in"):
                f(depth, K, src, cams, T, valid_in=bad)
        for bad in (torch.ones(2, 3, 5, 6, dtype=torch.bool), torch.ones(2, 3, 5, 7), torch.ones(2, 1, 5, 7, dtype=torch.bool), torch.ones(3, 5, 7, dtype=torch.bool), "m"):
            with pytest.raises(ValueError, match=f"{fn}: src_masks"):
                f(depth, K, src, cams, T, src_masks=bad)
        with pytest.raises(NotImplementedError):
            f(depth, K, src, [K, object(), K], T)
        # well-formed arguments on the CPU: the HIP kernels are the only implementation
        eucm = cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))
        opencv = cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12))
        for args, kw in (((depth, K, src, cams, T), {}), ((depth[:, 0], eucm, src.double(), (K, opencv, eucm), T[:, :3]), dict(min_views=0)),
                         ((depth, opencv, src, cams, torch.eye(4).repeat(2, 3, 1, 1)), dict(px_tol=0, rel_tol=0, min_views=3, return_views=True)),
                         ((depth, K, src, cams, torch.eye(4)[:3].repeat(2, 3, 1, 1)),
                          dict(valid_in=torch.ones(2, 4, 6, dtype=torch.bool), src_masks=torch.ones(2, 3, 5, 7, dtype=torch.uint8), return_errors=True))):
            with pytest.raises(RuntimeError, match="GPU"):
                f(*args, **kw)
    for name in ("depth_consistency", "depth_consistency_composition", "invert_rigid"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(consistency, name)
    doc = consistency.depth_consistency.__doc__
    assert "depth_consistency_composition" in doc and "OPENCV or Fisheye624" in doc and "launches" in doc and "invert_rigid" in doc


def _ulps(a, b):
    """the distance of two fp32 arrays in units in the last place of b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


def test_invert_rigid():
    """[R^T | -(R^T t)] by its stated arithmetic; the inverse of the inverse stays within 2 fp32 ulp of T for rotations built from exactly
    representable entries -- the 24 proper signed axis permutations, the only rotations all of whose entries are binary fractions -- with
    translations in sixteenths, where invert_rigid is also the exact inverse.  For the small general rotations of the scenes, whose fp32
    entries are only nearly orthogonal, R comes back bit-equal and t within 2 ulp of its largest component (an element near 0 has no
    ulp of its own to be measured in)."""
    from unidepth_amd import consistency
    import itertools
    mats = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                mats.append(R)
    assert len(mats) == 24
    g = np.random.RandomState(9500)
    T = np.zeros((24, 4, 4), np.float32)
    T[:, :3, :3] = np.stack(mats)
    T[:, :3, 3] = g.randint(-64, 65, size=(24, 3)) / 16.0
    T[:, 3, 3] = 1.0
    Tt = torch.from_numpy(T)
    inv = consistency.invert_rigid(Tt)
    assert inv.shape == Tt.shape and inv.dtype == torch.float32
    assert torch.equal(inv @ Tt, torch.eye(4).expand(24, 4, 4))                      # exact arithmetic: the true inverse
    back = consistency.invert_rigid(inv)
    assert _ulps(back.numpy(), T)[np.abs(T) > 0].max() <= 2 and np.array_equal(back.numpy() == 0, T == 0)
    # the 3x4 form, batched [B,V,3,4], and the stated order of the operations
    P = torch.from_numpy(np.stack([cc._pose(g) for _ in range(6)]).reshape(2, 3, 3, 4))
    inv = consistency.invert_rigid(P)
    assert inv.shape == P.shape and torch.equal(inv[..., :3], P[..., :3].transpose(-1, -2))
    R, t = P[..., :3].numpy(), P[..., 3].numpy()
    want = -((R[..., 0, :] * t[..., 0:1] + R[..., 1, :] * t[..., 1:2]) + R[..., 2, :] * t[..., 2:3])
    assert want.dtype == np.float32 and np.array_equal(inv[..., 3].numpy(), want)
    # rotations: twice inverted, R is bit-equal and t within 2 ulp of its largest component
    back = consistency.invert_rigid(inv)
    assert torch.equal(back[..., :3], P[..., :3])
    scale = np.spacing(np.abs(t).max(axis=-1, keepdims=True).astype(np.float32))
    assert (np.abs(back[..., 3].numpy().astype(np.float64) - t) / scale).max() <= 2
    for bad in (torch.eye(3), torch.eye(4).double(), torch.rand(4), "T"):
        with pytest.raises(ValueError, match="invert_rigid"):
            consistency.invert_rigid(bad)
