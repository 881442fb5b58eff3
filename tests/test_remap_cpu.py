"""remap / undistort / overlap_mask without a GPU (unidepth_amd/remap.py, include/unidepth_hip.h UdRemap / UdOverlapMask): the functions of
csrc/remap_taps.h compiled for the host and run point by point under the host sanitizers (tests/remap_host/remap_host.cpp, a stand-alone
program) against the numpy fp32 restatement of tools/make_golden_remap.py, bit for bit, in every mode, padding and flag, on the special
coordinates and on the golden cases; the golden file against the restatements and its own seeds; every refusal
of both entry points and the Python argument errors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import host_program
import remap_common as common

ROOT = common.ROOT
rm, cp = common.rm, common.cp
MODE_ID = {"nearest": 0, "bilinear": 1}
PAD_ID = {"zeros": 0, "border": 1}


# ---- the header functions, compiled for the host with the sanitizers ------------------------------------------------------------------

@pytest.fixture(scope="module")
def remap_host(tmp_path_factory):
    return host_program.build(tmp_path_factory, "remap_host")


def _run(exe, args, blobs, n_out):
    return host_program.run(exe, args, blobs, [n_out])[0]


def _host_remap(exe, src, uv, cfg, mask, cv, out_u8=False, uv_rows=True, out_rows=True, B=None):
    """arrays sized exactly to their contents: an index that escapes is an AddressSanitizer report"""
    mode, padding, normalize, _, _ = cfg
    B = max(src.shape[0], uv.shape[0]) if B is None else B
    _, Cc, Hs, Ws = src.shape
    N = uv.shape[1]
    u8 = src.dtype == np.uint8
    coords = uv if uv_rows else uv.transpose(0, 2, 1)
    blobs = [np.ascontiguousarray(src).tobytes()] + ([np.ascontiguousarray(mask).tobytes()] if mask is not None else []) + \
            [np.ascontiguousarray(coords, np.float32).tobytes()] + ([np.ascontiguousarray(cv).tobytes()] if cv is not None else [])
    osz = 1 if out_u8 else 4
    raw = _run(exe, ["remap", MODE_ID[mode], PAD_ID[padding], int(normalize), int(u8), int(out_u8), int(uv_rows), int(out_rows), B, Cc, Hs, Ws, N,
                     src.shape[0], uv.shape[0], 0 if mask is None else mask.shape[0], int(cv is not None), 1], blobs, B * N * Cc * osz + B * N)
    out = np.frombuffer(raw[:B * N * Cc * osz], dtype=np.uint8 if out_u8 else np.float32)
    out = out.reshape(B, N, Cc) if out_rows else np.ascontiguousarray(out.reshape(B, Cc, N).transpose(0, 2, 1))
    return out, np.frombuffer(raw[B * N * Cc * osz:], dtype=np.uint8).reshape(B, N).astype(bool)


@pytest.mark.parametrize("name", list(common.SETS))
def test_host_build_equals_restatement_in_every_configuration(remap_host, name):
    """every point of every set -- regular points up to a quarter of the image outside it, NaN, +-inf, +-1e30, -0.0, exactly 0, exactly
    the size and one ulp beyond, exact half-integers, the rint ties -- in all 32 configurations: bit-equal values and validity, and no
    sanitizer report (the program's exit status)"""
    d = common.inputs(name)
    u8 = d["src"].dtype == np.uint8
    for cfg in common.CONFIGS:
        mask, cv = (d["mask"] if cfg[3] else None), (d["cv"] if cfg[4] else None)
        for out_u8 in ((False, True) if u8 else (False,)):
            want, wvalid = common.want(name, cfg, out_u8)
            rows = cfg[2] == cfg[3]                                  # both layouts get every mode and padding
            got, valid = _host_remap(remap_host, d["src"], d["uv"], cfg, mask, cv, out_u8, uv_rows=rows, out_rows=rows, B=d["B"])
            assert common.same_bits(got, want), (name, cfg, out_u8)
            assert np.array_equal(valid, wvalid), (name, cfg, out_u8)


def test_special_coordinates_are_there_and_behave():
    """the special set holds what it is there for, and the restatement's answers on it are the documented ones"""
    f = np.float32
    for Hs, Ws in rm.SIZES:
        sp = rm.special_points(Hs, Ws)[0]
        u = sp[:, 0]
        assert np.isnan(u).any() and np.isposinf(u).any() and np.isneginf(u).any() and (u == f(1e30)).any() and (u == f(-1e30)).any()
        assert (np.signbit(u) & (u == 0)).any() and ((u == 0) & ~np.signbit(u)).any() and (u == f(Ws)).any() and (u == np.nextafter(f(Ws), f(np.inf))).any()
        assert (u == f(0.5)).any() and (u == f(Ws - 0.5)).any() and (u == f(2.0)).any() and (u == f(3.0)).any()
        src = rm.source(Hs, Ws, 2, 1, 99)
        for mode in rm.MODES:
            for padding in rm.PADDINGS:
                out, valid = rm.remap(src, sp[None], mode, padding)
                bad = ~np.isfinite(sp).all(axis=1)
                assert (out[0][bad] == 0).all() and not valid[0][bad].any()
                inside = (sp[:, 0] >= 0) & (sp[:, 0] <= Ws) & (sp[:, 1] >= 0) & (sp[:, 1] <= Hs) & ~bad
                # no mask: every inside point has a live tap, but for nearest / zeros at u = Ws exactly where Ws is even: x = Ws - 0.5 ties
                # to the even pixel Ws, which does not exist (grid_sample's nearest returns its padding there too)
                edge = (mode, padding) == ("nearest", "zeros") and ((sp[:, 0] == Ws) & (Ws % 2 == 0) | (sp[:, 1] == Hs) & (Hs % 2 == 0))
                assert np.array_equal(valid[0], inside & ~edge), (mode, padding)
                far = (np.abs(sp) >= f(1e30)).any(axis=1) & ~bad
                if padding == "zeros":
                    assert far.any() and (out[0][far] == 0).all()
                else:
                    assert (out[0][far] > 0).any()                                 # the border's value, valid 0
    # the rint ties of nearest: x = 0.5, 1.5, 2.5 -> pixels 0, 2, 2
    src = np.arange(12, dtype=np.float32).reshape(1, 1, 2, 6)
    uv = np.array([[[1.0, 0.5], [2.0, 0.5], [3.0, 0.5], [0.0, 0.5], [6.0, 0.5]]], np.float32)
    out, valid = rm.remap(src, uv, "nearest", "zeros")
    assert out[0, :, 0].tolist() == [0.0, 2.0, 2.0, 0.0, 0.0] and valid[0].tolist() == [True, True, True, True, False]
    # above: x = -0.5 rounds to -0, pixel 0; x = 5.5 rounds to 6: no tap, so not valid.  border clamps x to [0, 5] first
    out, valid = rm.remap(src, uv, "nearest", "border")
    assert out[0, :, 0].tolist() == [0.0, 2.0, 2.0, 0.0, 5.0] and valid[0].all()
    # normalised bilinear over a hole: the live taps' weighted mean, 0 and invalid where no tap is live
    mask = np.ones((1, 2, 6), np.uint8)
    mask[0, :, 2:4] = 0
    uv = np.array([[[2.0, 1.0], [3.0, 1.0], [4.0, 1.0]]], np.float32)
    out, valid = rm.remap(src, uv, "bilinear", "zeros", src_mask=mask, normalize=True)
    assert out[0, :, 0].tolist() == [4.0, 0.0, 7.0] and valid[0].tolist() == [True, False, True]


def test_host_build_point_counts_and_centres(remap_host):
    """the first n points of a set (the golden grid_sample cases' counts follow on the GPU); exact pixel centres return the source's bits
    in all four mode / padding pairs"""
    name = "f32_37x53_c3_b3"
    d = common.inputs(name)
    cfg = ("bilinear", "zeros", True, True, True)
    for n in common.POINT_COUNTS:
        want, wvalid = common.want(name, cfg, False, n)
        got, valid = _host_remap(remap_host, d["src"], d["uv"][:, :n], cfg, d["mask"], d["cv"][:, :n])
        assert common.same_bits(got, want) and np.array_equal(valid, wvalid), n
    for name in ("f32_48x64_c1_b3_shared_uv", "f32_37x53_c5_b1_centres"):
        d = common.inputs(name)
        Hs, Ws = d["src"].shape[-2:]
        src_rows = d["src"].reshape(d["src"].shape[0], d["src"].shape[1], Hs * Ws).transpose(0, 2, 1)
        for mode in rm.MODES:
            for padding in rm.PADDINGS:
                got, valid = _host_remap(remap_host, d["src"], d["uv"], (mode, padding, False, False, False), None, None, B=d["B"])
                assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(src_rows).view(np.uint32)) and valid.all(), (name, mode, padding)


def test_host_build_overlap_equals_restatement(remap_host):
    fields = dict(common.overlap_fields(), nan_37x53=rm.nan_field())
    for name, uv in fields.items():
        B, _, H, W = uv.shape
        raw = _run(remap_host, ["overlap", B, H, W], [np.ascontiguousarray(uv, np.float32).tobytes()], B * H * W)
        got = np.frombuffer(raw, dtype=np.uint8).reshape(B, 1, H, W)
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), rm.overlap(uv)), name
    nan = rm.overlap(rm.nan_field())
    assert not nan[0, 0, 3, 4] and not nan[0, 0, 20, 30] and not nan[0, 0, 36, 52] and not nan[0, 0, 0, 0] and not nan[0, 0, 11, 17]


# ---- the golden file ------------------------------------------------------------------------------------------------------------------

def test_golden_has_every_case_and_its_conditions_hold():
    g = common.golden()
    want = [f"{n}.{k}" for n in rm.GS_CASES for k in ["sum"] + [f"{m}.{p}" for m in rm.MODES for p in rm.PADDINGS]]
    want += ["referr." + k for k in rm.MODES + ("undistort",)]
    want += [n + ".overlap" for n in rm.OV_FIELDS] + [f"proj_{n}.{k}" for n in rm.OV_PROJECTED for k in ("overlap", "uv")]
    want += [f"{n}.{k}" for n in rm.UD_CASES for k in ("sum", "out", "mask")]
    assert sorted(g) == sorted(want)
    assert os.path.getsize(rm.GOLDEN) <= os.path.getsize(cp.GOLDEN)
    bars = common.bars()
    for name in rm.GS_CASES:
        src, uv = rm.gs_inputs(name)
        H, W, Cc, B, N = rm.GS_CASES[name]
        assert list(g[name + ".sum"]) == [rm.checksum(src), rm.checksum(uv)]        # the seeded inputs the arrays were made from
        assert src.min() >= 0 and src.max() <= 5 and src.shape == (B, Cc, H, W)
        d = np.abs(uv.astype(np.float64) - np.rint(uv.astype(np.float64)))
        assert d.min() >= rm.TIE_MARGIN                                              # clear of the rint ties and of the edges of valid
        size = np.array([W, H])
        assert (uv < 0).any() and (uv > size).any() and (uv >= -0.25 * size).all() and (uv <= 1.25 * size).all()
        for mode in rm.MODES:
            for padding in rm.PADDINGS:
                ref = g[f"{name}.{mode}.{padding}"]
                r64 = rm.remap(src, uv, mode, padding, dtype=np.float64)[0]
                r32 = rm.remap(src, uv, mode, padding)[0]
                assert ref.shape == r32.shape == (B, N, Cc)
                e = float(rm.value_error(r32 - ref, r64).max())
                print(f"{name} {mode} {padding}: restatement vs grid_sample {e:.3e}, bar {bars[mode]:.3e}")
                assert e <= bars[mode], (name, mode, padding, e)                     # every regular point, none excluded
                assert float(rm.value_error(ref - r64, r64).max()) <= float(g["referr." + mode]) * (1 + 1e-9)
    for mode in rm.MODES:
        e = float(g["referr." + mode])
        assert 0 <= e < 1e-3 and rm.bar(e) == max(4 * e, 8 * 2.0 ** -24)
    assert float(g["referr.bilinear"]) > 0 and float(g["referr.undistort"]) > 0


def test_overlap_restatement_against_the_reference_masks():
    """the reference's own mask_overlap_projection (stored): equal on every pixel the fp64 restatement keeps 1e-3 px from the decision
    that would change it, at most 1 % of a case's pixels left out; the fields are not trivially all-True"""
    g = common.golden()
    shares = {}
    for name, uv in common.overlap_fields().items():
        margin = []
        m64 = rm.overlap(uv, np.float64, margin)
        keep = margin[0] >= rm.OVERLAP_MARGIN
        ref = common.unpack(g[name + ".overlap"], m64.shape)
        for b in range(uv.shape[0]):
            assert (~keep[b]).mean() <= rm.BAND_CAP, (name, b)
        assert np.array_equal(ref[keep], m64[keep]) and np.array_equal(rm.overlap(uv)[keep], ref[keep]), name
        shares[name] = float((~ref).mean())
    assert sum(s > 0.2 for s in shares.values()) >= 4 and min(shares.values()) == 0.0, shares


def test_undistort_restatement_against_the_reference_chain():
    """unproject -> project -> remap restated in fp32 against the reference's chain (stored): masks equal and values within the measured
    bar on every pixel outside the band (fp64 coordinate 1e-2 px from the border or depth from 0), the band at most 1 % of a case"""
    g = common.golden()
    bar = common.bars()["undistort"]
    for name in rm.UD_CASES:
        assert list(g[name + ".sum"]) == [rm.checksum(rm.ud_inputs(name)[0])]
        uv64, _, o64, v64, d64 = rm.ud_chain(name, np.float64)
        _, _, o32, v32, _ = rm.ud_chain(name, np.float32)
        keep = ~rm.ud_band(uv64, d64)
        ref, rmask = g[name + ".out"], common.unpack(g[name + ".mask"], v64.shape)
        for b in range(keep.shape[0]):
            assert (~keep[b]).mean() <= rm.BAND_CAP, (name, b)
        assert np.array_equal(v32[keep], rmask[keep]), name
        both = keep & rmask & v32
        e = float(rm.value_error(o32 - ref, o64)[both].max())
        print(f"{name}: fp32 restatement vs the reference's chain {e:.3e}, bar {bar:.3e}")
        assert both.mean() > 0.5 and e <= bar, (name, e, bar)
    assert not common.unpack(g["ud_six_to_opencv.mask"], v64.shape).all()


def _reference_available():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return ref_loader.available()


@pytest.mark.skipif(not _reference_available(), reason="the reference tree is not present")
def test_golden_regenerates_bit_for_bit():
    """every array of the golden file again from the seeds, torch's CPU grid_sample and the reference's own classes: the same bytes"""
    out, _ = rm.build()
    g = common.golden()
    assert sorted(out) == sorted(g)
    for k, v in out.items():
        a, b = np.asarray(v), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_every_refusal():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_remap(None, None) < 0 and "null descriptor" in lib.ud_last_error().decode()
    assert lib.ud_overlap_mask(None, None) < 0 and "null descriptor" in lib.ud_last_error().decode()

    def call(**kw):
        d = _lib.UdRemap()
        base = dict(src=16, src_mask=None, uv=16, coord_valid=None, out=16, valid=None, batch_stride=70, point_stride=2, comp_stride=1,
                    n_points=35, B=2, C=3, Hs=5, Ws=7, mode=1, padding=0, normalize=0, src_u8=0, out_u8=0, out_rows=1, src_shared=0, mask_shared=0)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.ud_remap(C.byref(d), None), lib.ud_last_error().decode()
    big = 2 ** 31 - 256
    for kw, msg in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes"), (dict(C=0), "bad sizes"), (dict(Hs=0), "bad sizes"),
                    (dict(Ws=-1), "bad sizes"), (dict(n_points=0), "bad sizes"), (dict(n_points=-3), "bad sizes"),
                    (dict(n_points=big, C=1), "too large"), (dict(n_points=big // 2, C=2), "too large"), (dict(Hs=1 << 16, Ws=1 << 15, C=1), "too large"),
                    (dict(Hs=1 << 15, Ws=1 << 15, C=2), "too large"), (dict(Hs=2 ** 31 - 1, Ws=2 ** 31 - 1, C=2 ** 31 - 1), "too large"),
                    (dict(src=None), "null pointer"), (dict(uv=None), "null pointer"), (dict(out=None), "null pointer"),
                    (dict(point_stride=0), "bad strides"), (dict(comp_stride=0), "bad strides"), (dict(batch_stride=-1), "bad strides"),
                    (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(padding=2), "unknown padding"),
                    (dict(padding=-1), "unknown padding"), (dict(out_u8=1), "uint8 output")):
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)

    def ocall(**kw):
        d = _lib.UdOverlapMask()
        base = dict(uv=16, mask=16, B=2, H=5, W=7)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.ud_overlap_mask(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in ((dict(B=0), "bad sizes"), (dict(B=_lib.UD_RECON_MAX_B + 1), "bad sizes"), (dict(H=1), "bad sizes"), (dict(W=1), "bad sizes"),
                    (dict(H=0), "bad sizes"), (dict(W=-4), "bad sizes"), (dict(H=1 << 16, W=1 << 15), "too large"),
                    (dict(uv=None), "null pointer"), (dict(mask=None), "null pointer")):
        rc, err = ocall(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import importlib
    import unidepth_amd
    from unidepth_amd import cameras
    module = importlib.import_module("unidepth_amd.remap")
    f = module.remap
    src, uv, rows = torch.rand(2, 3, 5, 7), torch.rand(2, 2, 4, 6), torch.rand(2, 11, 2)
    for kw in (dict(mode="bicubic"), dict(padding="reflection"), dict(out_dtype=torch.float16), dict(out_dtype=torch.uint8)):
        with pytest.raises(ValueError):
            f(src, uv, **kw)
    for bad in (torch.rand(3, 5, 7), torch.rand(2, 0, 5, 7), torch.ones(2, 3, 5, 7, dtype=torch.int32), "src"):
        with pytest.raises(ValueError, match="src"):
            f(bad, uv)
    for bad in (torch.rand(2, 3, 4, 6), torch.rand(2, 11, 3), torch.rand(4, 6), torch.ones(2, 2, 4, 6, dtype=torch.int64), torch.rand(0, 2, 4, 6),
                torch.rand(2, 0, 2), "uv"):
        with pytest.raises(ValueError, match="uv"):
            f(src, bad)
    for bad in (torch.ones(2, 1, 5, 6, dtype=torch.bool), torch.ones(2, 1, 5, 7), torch.ones(2, 2, 5, 7, dtype=torch.bool), torch.ones(5, 7, dtype=torch.bool)):
        with pytest.raises(ValueError, match="src_mask"):
            f(src, uv, src_mask=bad)
    for bad in (torch.ones(2, 1, 4, 5, dtype=torch.bool), torch.ones(2, 4, 6), torch.ones(2, 24, 1, dtype=torch.bool), torch.ones(24, dtype=torch.bool)):
        with pytest.raises(ValueError, match="coord_valid"):
            f(src, uv, coord_valid=bad)
    with pytest.raises(ValueError, match="coord_valid"):
        f(src, rows, coord_valid=torch.ones(2, 1, 11, dtype=torch.bool))
    with pytest.raises(ValueError, match="images"):
        f(src, torch.rand(3, 2, 4, 6))                                             # 2 sources, 3 coordinate sets
    with pytest.raises(ValueError, match="images"):
        f(src, uv, src_mask=torch.ones(3, 1, 5, 7, dtype=torch.bool))
    with pytest.raises(ValueError, match="images"):
        f(src[:1], uv, coord_valid=torch.ones(3, 4, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="at most"):
        f(src[:1], torch.rand(257, 1, 2))
    # well-formed arguments on the CPU: the HIP kernels are the only implementation
    for args, kw in (((src, uv), {}), ((src, rows), dict(mode="nearest", padding="border", return_mask=True)), ((src[:1], uv), {}),
                     ((src.to(torch.uint8), uv), dict(out_dtype=torch.uint8)), ((src, uv), dict(src_mask=torch.ones(2, 1, 5, 7, dtype=torch.bool),
                                                                                                  coord_valid=torch.ones(2, 4, 6, dtype=torch.bool), normalize=True))):
        with pytest.raises(RuntimeError, match="GPU"):
            f(*args, **kw)
    g = module.overlap_mask
    for bad in (torch.rand(2, 3, 5, 7), torch.rand(2, 5, 7), torch.rand(2, 2, 1, 7), torch.rand(2, 2, 5, 1), torch.rand(0, 2, 5, 7),
                torch.ones(2, 2, 5, 7, dtype=torch.int32), torch.rand(257, 2, 2, 2), "uv"):
        with pytest.raises(ValueError):
            g(bad)
    with pytest.raises(RuntimeError, match="GPU"):
        g(torch.rand(2, 2, 5, 7))
    h = module.undistort
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    for bad in (torch.rand(3, 5, 7), torch.rand(2, 0, 5, 7), "src"):
        with pytest.raises(ValueError, match="src"):
            h(bad, K)
    for shp in ((0, 7), (5,), "hw"):
        with pytest.raises(ValueError, match="out_shape"):
            h(src, K, out_shape=shp)
    with pytest.raises(ValueError, match="images"):
        h(src, cameras.BatchCamera([cameras.Pinhole(K)] * 3))
    with pytest.raises(NotImplementedError):
        h(src, object())
    with pytest.raises(RuntimeError, match="GPU"):
        h(src, K)
    for cls in (cameras.Pinhole, cameras.EUCM, cameras.Spherical, cameras.OPENCV, cameras.Fisheye624, cameras.MEI, cameras.BatchCamera):
        assert callable(cls.get_overlap_mask) and cls.overlap_mask is None
    assert cameras.Pinhole(K).get_overlap_mask() is None
    for name in ("remap", "undistort", "overlap_mask"):
        assert name in unidepth_amd.__all__ and getattr(module, name) is not None
    assert unidepth_amd.undistort is module.undistort and unidepth_amd.overlap_mask is module.overlap_mask
    assert callable(unidepth_amd.remap) and unidepth_amd.remap.remap is module.remap           # the module answers a call as its function
    doc = module.undistort.__doc__
    assert "RESAMPLED, not converted" in doc and "Spherical" in doc and "caller's business" in doc
