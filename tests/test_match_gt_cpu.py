"""match_gt / match_intrinsics / forward_test without a GPU (unidepth_amd/matching.py, include/unidepth_hip.h UdMatchGt): the numpy
restatement of tools/make_golden_match_gt.py against the reference's own arrays (tests/golden/match_gt.npz) and against itself in fp64,
the C-ABI's descriptor and argument checks, the Python argument errors, and the dict dispatch of the model classes."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import layout_guard as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_match_gt", os.path.join(ROOT, "tools", "make_golden_match_gt.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

_CACHE = {}


def _case(name):
    """inputs, both restatements and the per-element bound of a case, computed once.
    bound = term_rounding(mag, 4) + term_coord(max source coordinate, sum |taps|): four products and three sums in fp32 on the
    magnitude of the same expression, plus source coordinates / weights computed in fp32 -- a coordinate of at most max(hu, wu) (the
    largest window side of the batch) moves the result by its rounding times the taps' absolute sum."""
    if name not in _CACHE:
        src, p1, p2, K, (H2, W2) = mg.case_inputs(name)
        B, _, h1, w1 = src.shape
        r64 = torch.from_numpy(mg.restate(src, H2, W2, p1, p2, dtype=np.float64))
        r32 = torch.from_numpy(mg.restate(src, H2, W2, p1, p2, dtype=np.float32))
        mag = torch.from_numpy(mg.restate(np.abs(src), H2, W2, p1, p2, dtype=np.float64))
        taps = torch.from_numpy(mg.restate(src, H2, W2, p1, p2, dtype=np.float64, what="tapsum"))
        coord = max(max(h1 - int(p1[b, 2]) - int(p1[b, 3]), w1 - int(p1[b, 0]) - int(p1[b, 1])) for b in range(B))
        bound = lg.term_rounding(mag, 4) + lg.term_coord(coord, taps)
        _CACHE[name] = dict(src=src, p1=p1, p2=p2, K=K, H2=H2, W2=W2, r64=r64, r32=r32, bound=bound)
    return _CACHE[name]


def test_golden_has_every_case():
    g = np.load(mg.GOLDEN)
    assert sorted(g.files) == sorted([n + ".out" for n in mg.GOLDEN_CASES] + [n + ".K" for n in mg.GOLDEN_CASES])
    for name in mg.GOLDEN_CASES:
        B, Cn, h1, w1, H2, W2, _, _ = mg.CASES[name]
        assert g[name + ".out"].dtype == np.float32 and g[name + ".out"].shape == (B, Cn, H2, W2)
        assert g[name + ".K"].dtype == np.float32 and g[name + ".K"].shape == (B, 3, 3)
    assert os.path.getsize(mg.GOLDEN) < 200 * 1024
    shapes = {c[2:6] for c in mg.CASES.values()}
    assert {(28, 42, 37, 53), (42, 56, 20, 31), (14, 70, 33, 17), (28, 42, 63, 257), (98, 126, 480, 640), (518, 518, 375, 1242)} <= shapes


@pytest.mark.parametrize("name", mg.GOLDEN_CASES)
def test_reference_golden_within_bound_of_fp64_restatement(name):
    """the reference's own match_gt output against the fp64 restatement, every element; exact zeros in the target border"""
    c = _case(name)
    ref = torch.from_numpy(np.load(mg.GOLDEN)[name + ".out"])
    w = lg.assert_bound(ref, c["r64"], c["bound"], name=name)
    print(f"{name}: reference uses {w:.3f} of the bound")
    outside = c["r64"] == 0
    assert bool((ref[outside] == 0).all())


@pytest.mark.parametrize("name", list(mg.CASES))
def test_fp32_restatement_within_bound_of_fp64(name):
    """the kernel's definition (fp32, every operation rounded separately) against fp64, up to the 518 x 518 -> 375 x 1242 case; the
    torch composition a user would write stays inside the same bound (it is NOT bit-equal to the fp32 restatement: it associates the
    four products differently)"""
    c = _case(name)
    w32 = lg.assert_bound(c["r32"], c["r64"], c["bound"], name=name + " fp32 restatement")
    comp = mg.torch_composition(torch.from_numpy(c["src"]), c["H2"], c["W2"], c["p1"], c["p2"])
    wt = lg.assert_bound(comp, c["r64"], c["bound"], name=name + " torch composition")
    print(f"{name}: fp32 restatement {w32:.3f}, torch composition {wt:.3f} of the bound")
    assert tuple(comp.shape) == tuple(c["r32"].shape)


def test_restatement_special_cases():
    """identity windows are bit copies (with and without mul), a broadcast source repeats, 1 x 1 windows spread one value"""
    rng = np.random.default_rng(5)
    src = rng.standard_normal((2, 2, 6, 9)).astype(np.float32)
    src[0, 0, 2, 3], src[1, 1, 4, 4] = -0.0, np.inf
    p1 = np.array([[1, 2, 0, 1], [3, 0, 1, 0]])
    out = mg.restate(src, 5, 6, p1, None)
    assert np.array_equal(out[0].view(np.int32), src[0, :, 0:5, 1:7].view(np.int32))
    assert np.array_equal(out[1].view(np.int32), src[1, :, 1:6, 3:9].view(np.int32))
    mul = rng.standard_normal((2, 1, 6, 9)).astype(np.float32)
    outm = mg.restate(src[:1], 5, 6, p1, None, mul=mul)
    assert np.array_equal(outm[1].view(np.int32), (src[0] * mul[1])[:, 1:6, 3:9].view(np.int32))
    one = mg.restate(src, 4, 5, np.array([[8, 0, 0, 5], [0, 8, 5, 0]]), np.array([[1, 1, 1, 1], [0, 0, 0, 0]]))
    assert np.array_equal(one[0, :, 1:3, 1:4], np.broadcast_to(src[0, :, 0:1, 8:9], (2, 2, 3)))
    assert (one[0, :, 0] == 0).all() and (one[0, :, :, 0] == 0).all() and (one[0, :, 3] == 0).all() and (one[0, :, :, 4] == 0).all()
    assert np.array_equal(one[1], np.broadcast_to(src[1, :, 5:6, 0:1], (2, 4, 5)))


@pytest.mark.parametrize("name", mg.GOLDEN_CASES)
def test_intrinsics_restatement_equals_reference_golden(name):
    c = _case(name)
    got = mg.restate_intrinsics(c["K"], c["src"].shape[-2:], (c["H2"], c["W2"]), c["p1"], c["p2"])
    ref = np.load(mg.GOLDEN)[name + ".K"]
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
    assert np.array_equal(got[:, 0, 1], c["K"][:, 0, 1]) and np.array_equal(got[:, 2], c["K"][:, 2])      # the other entries are copied


@pytest.mark.skipif(not os.path.isfile(mg.reference_path()), reason="reference tree not present (authoring machine only)")
def test_reference_rerun_reproduces_golden():
    fns = mg.reference_functions()
    g = np.load(mg.GOLDEN)
    for name in mg.GOLDEN_CASES:
        out, K = mg.reference_output(fns, name)
        # the resample inside the case's rounding bound of the stored array (torch's CPU kernel may contract products and sums into FMAs
        # on one machine and not on another); the intrinsics are scalar operations: exact
        lg.assert_bound(torch.from_numpy(out), torch.from_numpy(g[name + ".out"]).double(), _case(name)["bound"], name=name)
        np.testing.assert_array_equal(K, g[name + ".K"], err_msg=name)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------

def test_match_gt_is_not_a_launch_program_op():
    from unidepth_amd import _lib
    assert _lib.UD_MATCH_MAX_PLANES == 4
    assert not any(name.startswith("ud_program_add_match") for name in dir(_lib.lib))       # the op runs after the launch program


def test_match_gt_rejects_bad_descriptors_without_a_launch():
    """every refusal comes back before any HIP call: this runs on a machine without a GPU, the pointers are never followed"""
    from unidepth_amd import _lib
    lib = _lib.lib
    P = 0x1000                                      # stands for a device pointer

    def rc(planes=1, plane_kw=None, **kw):
        d = _lib.UdMatchGt()
        for i in range(min(planes, 4)):
            d.planes[i].src, d.planes[i].dst, d.planes[i].C, d.planes[i].src_batch_stride = P, P, 1, 35
        for k, v in (plane_kw or {}).items():
            setattr(d.planes[0], k, v)
        base = dict(n_planes=planes, B=2, h1=5, w1=7, H2=4, W2=9)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        r = lib.ud_match_gt(C.byref(d), None)
        return r, lib.ud_last_error().decode()

    r, msg = lib.ud_match_gt(None, None), lib.ud_last_error().decode()
    assert r < 0 and "null descriptor" in msg
    for args, word in ((dict(planes=5), "n_planes"), (dict(planes=-1), "n_planes"),
                       (dict(B=0), "bad sizes"), (dict(B=65536), "bad sizes"), (dict(h1=0), "bad sizes"), (dict(w1=-1), "bad sizes"),
                       (dict(H2=0), "bad sizes"), (dict(W2=0), "bad sizes"),
                       (dict(plane_kw=dict(src=None)), "null pointer"), (dict(plane_kw=dict(dst=None)), "null pointer"),
                       (dict(plane_kw=dict(C=0)), "bad plane"), (dict(plane_kw=dict(src_batch_stride=-1)), "bad plane"),
                       (dict(plane_kw=dict(dst=P + 2)), "bad plane"), (dict(plane_kw=dict(C=1 << 30), H2=4), "bad plane"),
                       (dict(K_in=P), "K_in and K_out"), (dict(K_out=P), "K_in and K_out"),
                       (dict(planes=0), "nothing to do")):
        r, msg = rc(**args)
        assert r < 0 and word in msg, (args, r, msg)


# ---- Python argument checks (all before a GPU is needed) -------------------------------------------------------------------------------

def test_match_gt_argument_errors():
    from unidepth_amd import match_gt, match_intrinsics
    t1, t2 = torch.zeros(2, 1, 6, 8), torch.zeros(2, 1, 5, 7)
    K = torch.eye(3).repeat(2, 1, 1)
    for kw, word in ((dict(padding1=[(0, 0, 0, 0)]), "per image"),                                     # one row for two images
                     (dict(padding1=[(0, 0, 0, 0), (0, 0, 0)]), "per image"),
                     (dict(padding1=[(-1, 0, 0, 0), (0, 0, 0, 0)]), "negative"),
                     (dict(padding1=torch.tensor([[0, 0, 0, 0], [4, 4, 0, 0]])), "empty window"),      # 8 - 4 - 4 = 0 columns
                     (dict(padding1=[(0, 0, 3, 3), (0, 0, 0, 0)]), "empty window"),
                     (dict(padding2=[(0, 0, 0, 0), (0, 7, 0, 0)]), "empty window"),
                     (dict(padding2=[(0, 0, 0, -2), (0, 0, 0, 0)]), "negative"),
                     (dict(padding1=[(0.5, 0, 0, 0), (0, 0, 0, 0)]), "integer")):
        args = dict(padding1=None, padding2=None)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            match_gt(t1, t2, **args)
        with pytest.raises(ValueError, match=word):
            match_intrinsics(K, t1, t2, **args)
    with pytest.raises(ValueError, match="bilinear"):
        match_gt(t1, t2, None, None, mode="nearest")
    with pytest.raises(ValueError, match="batch sizes differ"):
        match_gt(t1, torch.zeros(3, 1, 5, 7), None, None)
    with pytest.raises(ValueError, match="batch sizes differ"):
        match_intrinsics(torch.eye(3).repeat(3, 1, 1), t1, t2, None, None)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        match_gt(t1[0], t2, None, None)
    with pytest.raises(ValueError, match=r"\[B,3,3\]"):
        match_intrinsics(torch.eye(4).repeat(2, 1, 1), t1, t2, None, None)
    # valid arguments on CPU tensors: the HIP kernel is the only implementation
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        match_gt(t1, t2, [(1, 1, 0, 0), (0, 0, 2, 2)], None)
    with pytest.raises(RuntimeError, match="GPU tensors expected"):
        match_intrinsics(K, t1, t2, None, torch.tensor([[1, 1, 0, 0], [0, 0, 2, 2]]))


def _v2():
    from oracle import synth
    from unidepth_amd import UniDepthV2
    return UniDepthV2(synth.load_config("vits14"))


def test_dict_argument_reaches_forward_test_and_tensor_reaches_infer(monkeypatch):
    from unidepth_amd import UniDepthV2
    model = _v2()
    seen = []
    real_ft, real_infer = UniDepthV2.forward_test, UniDepthV2.infer
    monkeypatch.setattr(UniDepthV2, "forward_test", lambda self, *a, **k: (seen.append("forward_test"), real_ft(self, *a, **k))[1])
    monkeypatch.setattr(UniDepthV2, "infer", lambda self, *a, **k: (seen.append("infer"), real_infer(self, *a, **k))[1])
    inputs = {"image": torch.zeros(2, 3, 28, 42), "depth": torch.zeros(2, 1, 9, 11)}
    metas = [{"paddings": (0, 0, 0, 0)}, {"paddings": (14, 0, 14, 0)}]
    for call in (lambda: model(inputs, metas), lambda: model.forward(inputs, metas), lambda: model(inputs=inputs, image_metas=metas)):
        with pytest.raises(RuntimeError, match="ROCm GPU only"):
            call()
    assert seen == ["forward_test"] * 3
    for call in (lambda: model(torch.zeros(3, 28, 42)), lambda: model.forward(torch.zeros(1, 3, 28, 42), None)):
        with pytest.raises(RuntimeError, match="ROCm GPU only"):
            call()
    assert seen == ["forward_test"] * 3 + ["infer"] * 2
    assert "paddings" not in inputs                                                            # the caller's dict is left alone


def test_forward_test_argument_errors():
    model = _v2()
    img, dep = torch.zeros(2, 3, 28, 42), torch.zeros(2, 1, 9, 11)
    for inputs, metas, word in (({"image": img}, None, "'image'"),
                                ({"image": torch.zeros(2, 3, 30, 42), "depth": dep}, None, "multiples"),
                                ({"image": img.to(torch.uint8), "depth": dep}, None, "float"),
                                ({"image": img, "depth": torch.zeros(3, 1, 9, 11)}, None, r"inputs\['depth'\]"),
                                ({"image": img, "depth": dep}, [{"paddings": (14, 0, 28, 0)}, {"paddings": (0, 0, 0, 0)}], "empty window"),
                                ({"image": img, "depth": dep, "paddings": torch.tensor([[0, 0, 14, 14], [0, 0, 0, 0]])}, None, "empty window"),
                                ({"image": img, "depth": dep}, [{"paddings": (0, 0, 0, 0)}], "per image")):
        with pytest.raises(ValueError, match=word):
            model.forward_test(inputs, metas)


def test_v1_forward_test_not_implemented():
    from oracle import synth_v1
    from unidepth_amd import UniDepthV1
    model = UniDepthV1(synth_v1.load_config_v1("cnvnxtl"))
    with pytest.raises(NotImplementedError, match="network-resolution"):
        model.forward_test({"image": torch.zeros(1, 3, 28, 28), "depth": torch.zeros(1, 1, 5, 5)}, [])
