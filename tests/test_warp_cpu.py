"""warp_camera without a GPU (unidepth_amd/warp.py, include/unidepth_hip.h UdWarpCamera): the fused per-pixel function of
csrc/warp_point.h compiled for the host and run under the host sanitizers (tests/warp_host/warp_host.cpp, a stand-alone program) against
the chain of the separate per-point functions of camera_models.h and remap_taps.h, bit for bit, for every model pair, mode, padding,
source type and transform of the GPU tests' cases, on the special values and on the known answer; the C-ABI's descriptor, every refusal
of the entry point and the Python argument errors.  Shared helpers: tests/warp_common.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import warp_common as wc

ROOT = wc.ROOT


@pytest.fixture(scope="module")
def warp_host(tmp_path_factory):
    return wc.build_host(tmp_path_factory)


# ---- the fused function against the chain, on the host --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in wc.DST_SETS if n != "iterative"])
def test_host_fused_equals_chain_for_every_model_pair(warp_host, name):
    """each closed-form destination model against the six source models (and the mixed batch), 37x53 <- 29x41, in both modes, both paddings,
    the three source / output types and the three transforms, all optional outputs on: the program exits non-zero when the fused function
    and the chain differ in one bit or a sanitizer reports.  The shares the GPU test asserts hold here too: at least a quarter of every
    image's pixels valid, at least a tenth not."""
    c = wc.case(name)
    seen = set()
    for tr in wc.TRANSFORMS:
        for kind in wc.KINDS:
            src, mask, norm, odt = wc.source_of(c, kind)
            for mode in wc.MODES:
                for pad in wc.PADDINGS:
                    r = wc.host_warp(warp_host, src, depth=c["depth"], params_dst=c["params_dst"], models_dst=c["models_dst"],
                                     params_src=c["params_src"], models_src=c["models_src"], T=wc.transform_of(c, tr), mode=mode, padding=pad,
                                     src_mask=mask, valid_in=c["valid_in"], normalize=norm, out_u8=odt == np.uint8, src_depth=c["src_depth"], tol=wc.TOL)
                    share = r["valid"].reshape(wc.B, -1).mean(axis=1)
                    assert share.min() >= 0.25 and share.max() <= 0.9, (name, tr, kind, mode, pad, share)
                    seen.add(bool(r["visible"].any()) and not bool(r["visible"].all()))
                    # a pixel whose destination depth is not positive, or whose valid_in is 0, samples nothing
                    dead = ~(c["depth"][:, 0] > 0) | (c["valid_in"] == 0)
                    assert dead.mean() > 0.08 and not r["valid"][dead].any() and not r["visible"][dead].any()
                    assert not r["out"][np.broadcast_to(dead[:, None], r["out"].shape)].any()
    assert seen == {True}


def test_host_points_form(warp_host):
    """the points form: no destination camera, every source model, with and without a transform"""
    c = wc.case("mixed")
    pts = wc.points_in_front(np.random.RandomState(9201), wc.B, wc.HO, wc.WO)
    for tr in ("none", "batch"):
        for kind, mode, pad in (("f32_c1_mask_norm", "bilinear", "zeros"), ("u8_c3", "nearest", "border"), ("u8_c3_f32", "bilinear", "border")):
            src, mask, norm, odt = wc.source_of(c, kind)
            r = wc.host_warp(warp_host, src, points=pts, params_src=c["params_src"], models_src=c["models_src"], T=wc.transform_of(c, tr), mode=mode,
                             padding=pad, src_mask=mask, valid_in=c["valid_in"], normalize=norm, out_u8=odt == np.uint8, src_depth=c["src_depth"], tol=wc.TOL)
            assert r["valid"].any() and not r["valid"].all()
            if tr == "none":                                                   # z <= 0: every model's depth test or in-image test fails
                behind = pts[:, 2] <= 0
                assert behind.mean() > 0.1 and not r["valid"][behind].any() and not r["out"][np.broadcast_to(behind[:, None], r["out"].shape)].any()


def test_host_special_values(warp_host):
    """the special values of warp_common.special_case: the program's own comparison with the chain, and out = 0, valid = visible = 0 on the
    pixels known to be dead"""
    c, depth, T, sd = wc.special_case()
    for name in ("mixed", "pinhole", "spherical"):
        cc = wc.case(name)
        for kind, mode, pad in (("f32_c1_mask_norm", "bilinear", "zeros"), ("u8_c3", "nearest", "border"), ("u8_c3_f32", "bilinear", "border"),
                                ("f32_c1_mask_norm", "nearest", "zeros")):
            src, mask, norm, odt = wc.source_of(c, kind)
            r = wc.host_warp(warp_host, src, depth=depth, params_dst=cc["params_dst"], models_dst=cc["models_dst"], params_src=c["params_src"],
                             models_src=c["models_src"], T=T, mode=mode, padding=pad, src_mask=mask, normalize=norm, out_u8=odt == np.uint8,
                             src_depth=sd, tol=wc.TOL)
            dead = np.zeros((wc.B, wc.HO, wc.WO), bool)
            dead[:, 0, 0:4] = True                                             # 0, negative, NaN, +inf: the point of +inf is not finite
            dead[:, 1, 0:3] = True                                             # +inf, -inf, -0.0
            dead[3:5] = True                                                   # z' = 0 and z' < 0
            assert not r["valid"][dead].any() and not r["visible"][dead].any() and not r["out"][np.broadcast_to(dead[:, None], r["out"].shape)].any()
            assert r["valid"][0].any() and r["valid"][5].any()
            fin = np.isfinite(depth[:, 0]) & (depth[:, 0] > 0)
            assert (r["proj_depth"][3][fin[3]] == 0).all() and (r["proj_depth"][4][fin[4]] < 0).all()


def test_host_known_answer(warp_host):
    k = wc.known_answer_inputs()

    def run(T, sd, mode):
        r = wc.host_warp(warp_host, k["src"], depth=k["depth"], params_dst=k["rows"], models_dst=(wc.PINHOLE,) * k["B"], params_src=k["rows"],
                         models_src=(wc.PINHOLE,) * k["B"], T=T, mode=mode, src_depth=sd, tol=wc.TOL)
        return r["out"], r["valid"], r["visible"]
    wc.check_known_answer(run)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_warp_descriptor_ends_with_the_model_arrays_and_has_no_float_field():
    from unidepth_amd import _lib
    fields = _lib.UdWarpCamera._fields_
    assert [n for n, _ in fields[-2:]] == ["model_dst", "model_src"]
    assert all(t in (C.c_void_p, C.c_longlong, C.c_int) for _, t in fields[:-2])


def test_every_refusal():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_warp_camera(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()

    def call(**kw):
        d = _lib.UdWarpCamera()
        base = dict(src=16, src_mask=None, src_depth=None, points=None, depth=16, params_dst=16, params_src=16, T=None, valid_in=None, out=16,
                    valid=None, visible=None, uv=None, proj_depth=None, B=2, C=3, Ho=4, Wo=6, Hs=5, Ws=7, nT=0, mode=1, padding=0, normalize=0,
                    src_u8=0, out_u8=0, src_shared=0, mask_shared=0, depth_shared=0, tol_bits=0)
        base.update(kw)
        dst, srcm = base.pop("dst", (1, 6)), base.pop("srcm", (4, 5))
        for k, v in base.items():
            setattr(d, k, v)
        for b, (md, ms) in enumerate(zip(dst, srcm)):
            d.model_dst[b], d.model_src[b] = md, ms
        return lib.ud_warp_camera(C.byref(d), None), lib.ud_last_error().decode()
    big = 2 ** 31 - 256
    for kw, msg, rc_want in (
            (dict(B=0), "bad sizes", -1), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes", -1), (dict(C=0), "bad sizes", -1), (dict(Ho=0), "bad sizes", -1),
            (dict(Wo=-1), "bad sizes", -1), (dict(Hs=0), "bad sizes", -1), (dict(Ws=-2), "bad sizes", -1),
            (dict(Ho=1 << 16, Wo=1 << 15, C=1), "too large", -1), (dict(Ho=1 << 15, Wo=1 << 15, C=2), "too large", -1), (dict(Ho=1, Wo=big, C=1), "too large", -1),
            (dict(Hs=1 << 16, Ws=1 << 15, C=1), "too large", -1), (dict(Hs=1 << 15, Ws=1 << 15, C=2), "too large", -1),
            (dict(Hs=2 ** 31 - 1, Ws=2 ** 31 - 1, C=2 ** 31 - 1), "too large", -1),
            (dict(points=16), "points or depth", -1), (dict(depth=None), "points or depth", -1),
            (dict(src=None), "null pointer", -1), (dict(params_src=None), "null pointer", -1), (dict(out=None), "null pointer", -1),
            (dict(params_dst=None), "null pointer", -1), (dict(visible=16), "null pointer", -1),
            (dict(mode=2), "unknown mode", -1), (dict(mode=-1), "unknown mode", -1), (dict(padding=2), "unknown padding", -1),
            (dict(padding=-1), "unknown padding", -1), (dict(out_u8=1), "uint8 output", -3),
            (dict(T=16, nT=0), "nT", -1), (dict(T=16, nT=3), "nT", -1),
            (dict(srcm=(0, 1)), "model tag", -1), (dict(srcm=(1, 7)), "model tag", -1), (dict(dst=(0, 1)), "model tag", -1), (dict(dst=(1, 9)), "model tag", -1),
            (dict(dst=(4, 1)), "iterative destination", -3), (dict(dst=(1, 5)), "iterative destination", -3)):
        rc, err = call(**kw)
        assert rc == rc_want and msg in err, (kw, rc, err)
    # the destination's tags are not read in the points form
    # (nothing else can be called here: a descriptor that passes every check would be launched)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import cameras, warp
    f = warp.warp_camera
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    src, depth, pts = torch.rand(2, 3, 5, 7), torch.rand(2, 1, 4, 6) + 1, torch.rand(2, 3, 4, 6)
    ok = dict(depth=depth, camera=K, src_camera=K)
    for kw, match in ((dict(mode="bicubic"), "mode"), (dict(padding="reflection"), "padding"), (dict(out_dtype=torch.float16), "out_dtype"),
                      (dict(out_dtype=torch.uint8), "out_dtype")):
        with pytest.raises(ValueError, match=match):
            f(src, **ok, **kw)
    for bad in (torch.rand(3, 5, 7), torch.rand(2, 0, 5, 7), torch.ones(2, 3, 5, 7, dtype=torch.int32), "src"):
        with pytest.raises(ValueError, match="src"):
            f(bad, **ok)
    with pytest.raises(ValueError, match="depth .* points"):
        f(src, src_camera=K)
    with pytest.raises(ValueError, match="depth .* points"):
        f(src, depth=depth, camera=K, points=pts, src_camera=K)
    with pytest.raises(ValueError, match="camera"):
        f(src, depth=depth, src_camera=K)
    with pytest.raises(ValueError, match="camera"):
        f(src, points=pts, camera=K, src_camera=K)
    for bad in (torch.rand(2, 2, 4, 6), torch.rand(4, 6), torch.ones(2, 1, 4, 6, dtype=torch.int64), torch.rand(0, 1, 4, 6), "depth"):
        with pytest.raises(ValueError, match="depth"):
            f(src, depth=bad, camera=K, src_camera=K)
    for bad in (torch.rand(2, 2, 4, 6), torch.rand(2, 24, 3), torch.ones(2, 3, 4, 6, dtype=torch.int32), torch.rand(0, 3, 4, 6), "points"):
        with pytest.raises(ValueError, match="points"):
            f(src, points=bad, src_camera=K)
    for bad in (torch.ones(2, 1, 5, 6, dtype=torch.bool), torch.ones(2, 1, 5, 7), torch.ones(2, 2, 5, 7, dtype=torch.bool), torch.ones(5, 7, dtype=torch.bool)):
        with pytest.raises(ValueError, match="src_mask"):
            f(src, src_mask=bad, **ok)
    for bad in (torch.ones(2, 1, 4, 5, dtype=torch.bool), torch.ones(2, 4, 6), torch.ones(2, 24, dtype=torch.bool), torch.ones(2, 2, 4, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="valid_in"):
            f(src, valid_in=bad, **ok)
    with pytest.raises(ValueError, match="together"):
        f(src, src_depth=torch.rand(2, 1, 5, 7), **ok)
    with pytest.raises(ValueError, match="together"):
        f(src, occlusion_tol=0.1, **ok)
    for bad in (torch.rand(2, 1, 5, 6), torch.ones(2, 1, 5, 7, dtype=torch.uint8), torch.rand(2, 2, 5, 7), "sd"):
        with pytest.raises(ValueError, match="src_depth"):
            f(src, src_depth=bad, occlusion_tol=0.1, **ok)
    for bad in (-0.1, float("nan"), float("inf"), 1e300, "tol"):
        with pytest.raises(ValueError, match="occlusion_tol"):
            f(src, src_depth=torch.rand(2, 1, 5, 7), occlusion_tol=bad, **ok)
    for bad in (torch.rand(3, 3), torch.rand(3, 3, 4), torch.eye(4)[None].expand(3, 4, 4), torch.rand(3, 4).double()):
        with pytest.raises(ValueError, match="transform"):
            f(src, transform=bad, **ok)
    with pytest.raises(ValueError, match="src of 3 images"):
        f(torch.rand(3, 3, 5, 7), **ok)
    with pytest.raises(ValueError, match="src_mask of 3 images"):
        f(src, src_mask=torch.ones(3, 1, 5, 7, dtype=torch.bool), **ok)
    with pytest.raises(ValueError, match="valid_in of 3 images"):
        f(src, valid_in=torch.ones(3, 4, 6, dtype=torch.bool), **ok)
    with pytest.raises(ValueError, match="src_depth of 3 images"):
        f(src, src_depth=torch.rand(3, 1, 5, 7), occlusion_tol=0.1, **ok)
    with pytest.raises(ValueError, match="src_camera of 3 images"):
        f(src, depth=depth, camera=K, src_camera=cameras.BatchCamera([cameras.Pinhole(K)] * 3))
    with pytest.raises(ValueError, match="camera of 3 images"):
        f(src, depth=depth, camera=K.expand(3, 3, 3), src_camera=K)
    with pytest.raises(ValueError, match="at most"):
        f(src[:1], depth=torch.rand(257, 1, 1, 1), camera=K, src_camera=K)
    with pytest.raises(NotImplementedError):
        f(src, depth=depth, camera=K, src_camera=object())
    # well-formed arguments on the CPU: the HIP kernel is the only implementation
    eucm = cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))
    opencv = cameras.OPENCV(torch.tensor([50.0, 51, 26, 18] + [0.0] * 12))
    T = torch.eye(4)[:3]
    for kw in (dict(depth=depth, camera=K, src_camera=K), dict(depth=depth[:, 0], camera=eucm, src_camera=opencv, transform=T),
               dict(points=pts, src_camera=cameras.BatchCamera([cameras.Pinhole(K), eucm]), transform=torch.eye(4)[None].expand(2, 4, 4).contiguous()),
               dict(depth=depth, camera=opencv, src_camera=K, mode="nearest", padding="border", return_mask=True, return_uv=True, return_depth=True),
               dict(depth=depth, camera=K, src_camera=K, src_mask=torch.ones(1, 1, 5, 7, dtype=torch.bool), valid_in=torch.ones(2, 4, 6, dtype=torch.bool),
                    normalize=True, src_depth=torch.rand(2, 1, 5, 7), occlusion_tol=0.1)):
        with pytest.raises(RuntimeError, match="GPU"):
            f(src, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        f(src.to(torch.uint8), out_dtype=torch.uint8, **ok)
    assert "warp_camera" in unidepth_amd.__all__ and unidepth_amd.warp_camera is warp.warp_camera
    assert unidepth_amd._WARP == ("warp_camera",)
    doc = f.__doc__
    assert "unprojection mask is deliberately" in doc and "return_mask=True" in doc and "five launches" in doc and "RESAMPLED, not converted" in doc
