"""CPU tests of the validation-input layer (unidepth_amd/testprep.py, include/unidepth_hip.h UdResizeAA): test_geometry and the numpy
restatement of ud_resize_aa (tools/make_golden_testprep.py) against the reference's own outputs in tests/golden/testprep.npz, the
descriptor mirror, the argument errors, and planted restatement defects that the comparison must catch.

Figures measured when the golden file was written (the reference = ATen's CPU antialias kernels in fp32 behind ContextCrop.crop):
  largest |reference - fp64 restatement| over the window cases: 1.049e-3 on uint8 sources (values 0..255), 1.510e-3 on the fp32 sources
  (values -64..320); the fp32 restatement deviates by at most 1.06e-3 / 1.6e-3 from the same fp64 values.
  share of pixels within 4e-3 of a half-integer (fp64): 0.05 % .. 0.98 % per plane set, except 9x11 -> 14x14 bilinear with 3.27 %
  (1.36 % of its pixels are EXACT ties, the same in fp32 and fp64); over both filters of that case, the unit the 3 % cap is applied
  to here, 2.04 %.  No byte of the reference differs from the fp32 restatement outside the excluded set, none by more than one level
  inside it, none at an exact tie."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_testprep", os.path.join(ROOT, "tools", "make_golden_testprep.py"))
tp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tp)

# largest deviation of the reference's own float arrays from the fp64 restatement over the golden window cases (measured: 1.049e-3 and
# 1.510e-3, see the module docstring); both implementations carry their own fp32 error, hence the factor 4 for the restatement
REF_DEV_U8, REF_DEV_F32 = 1.05e-3, 1.52e-3
TOL_U8, TOL_F32 = 4 * REF_DEV_U8, 4 * REF_DEV_F32
HALF_BAND = 4e-3
MAX_EXCLUDED = 0.03


@pytest.fixture(scope="module")
def golden():
    return np.load(tp.GOLDEN)


def _excluded(r64):
    return np.abs(r64 - np.floor(r64) - 0.5) <= HALF_BAND


def compare_bytes(r32, r64, ref_u8, defect=None):
    """the comparison of the uint8 image: (bytes differing outside the excluded set, largest level difference inside it, bytes
    differing at exact ties -- fp64 value k + 0.5 that the fp32 value equals --, excluded count)"""
    b = tp.to_u8(r32, defect)
    ex = _excluded(r64)
    tie = (r64 - np.floor(r64) == 0.5) & (r32.astype(np.float64) == r64)
    diff = b != ref_u8
    lvl = np.abs(b.astype(np.int64) - ref_u8.astype(np.int64))
    return int((diff & ~ex).sum()), int(lvl[ex].max()) if ex.any() else 0, int((diff & tie).sum()), int(ex.sum())


# ---- (a) geometry ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cons", tp.GEOMETRY_SETS)
@pytest.mark.parametrize("hw", tp.GEOMETRY_SIZES, ids=lambda s: "%dx%d" % s)
def test_geometry_equals_the_reference(golden, hw, cons):
    from unidepth_amd import testprep
    geo = testprep.test_geometry(hw, tp.IMAGE_SHAPE, tp.CONSTRAINTS[cons])
    k = f"geo.{cons}.{hw[0]}x{hw[1]}."
    assert geo.shape == tuple(golden[k + "shape"]) and geo.shape[0] % 14 == 0 and geo.shape[1] % 14 == 0
    assert geo.window == tuple(golden[k + "window"])
    assert geo.paddings == tuple(golden[k + "paddings"])
    assert geo.zoom == float(golden[k + "zoom"])
    top, left, height, width = geo.window
    assert top <= 0 and left <= 0 and top + height >= hw[0] and left + width >= hw[1]          # ctx = 1 never cuts the image


def test_geometry_of_the_project_configs_and_fixed_shapes():
    """the shipped configs carry the released shape_constraints (without `sample`: sampled, as in the reference's configs); with
    sample = False the rounded image_shape is the network shape"""
    import json
    from unidepth_amd import testprep
    with open(os.path.join(ROOT, "unidepth_amd", "configs", "config_v2_vitl14.json")) as f:
        cfg = json.load(f)

    def find(d):
        if isinstance(d, dict):
            if "shape_constraints" in d:
                return d["shape_constraints"]
            for v in d.values():
                r = find(v)
                if r is not None:
                    return r
        return None

    cons = find(cfg)
    assert cons is not None
    assert testprep.test_geometry((375, 1242), (518, 518), cons) == testprep.test_geometry((375, 1242), (518, 518), tp.CONSTRAINTS["v2"])
    fixed = dict(tp.CONSTRAINTS["v2"], sample=False)
    geo = testprep.test_geometry((480, 640), (470, 630), fixed)
    assert geo.shape == (476, 630) and geo.window == (-2, 0, 484, 640) and geo.zoom == 476 / 484


# ---- (b) the restatement against the reference's arrays ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tp.WINDOW_CASES))
def test_restatement_against_the_reference(golden, name):
    u8, f32, win, size = tp.case_inputs(name)
    excluded = total = 0
    for filt in tp.FILTERS:
        r64 = tp.restate(u8, win, size, filt, np.float64)
        r32 = tp.restate(u8, win, size, filt, np.float32)
        assert r32.dtype == np.float32
        ref = golden[f"{name}.{filt}.u8_f32"]
        dev_ref, dev = float(np.abs(ref - r64).max()), float(np.abs(r32 - r64).max())
        f64 = tp.restate(f32, win, size, filt, np.float64)
        dev_ref_f, dev_f = float(np.abs(golden[f"{name}.{filt}.f32"] - f64).max()), float(np.abs(tp.restate(f32, win, size, filt) - f64).max())
        bad, lvl, tie_bad, n_ex = compare_bytes(r32, r64, golden[f"{name}.{filt}.u8"])
        print(f"{name} {filt}: reference dev {dev_ref:.3e} / {dev_ref_f:.3e}, restatement dev {dev:.3e} / {dev_f:.3e}, "
              f"excluded {n_ex} of {r64.size} ({n_ex / r64.size:.4f})")
        assert dev_ref <= REF_DEV_U8 and dev_ref_f <= REF_DEV_F32          # the constants are the reference's own error
        assert dev <= TOL_U8 and dev_f <= TOL_F32
        assert bad == 0 and lvl <= 1 and tie_bad == 0
        excluded, total = excluded + n_ex, total + r64.size
    assert excluded <= MAX_EXCLUDED * total


def test_normalised_form_against_the_reference_steps(golden):
    """/255 and TF.normalize on the reference's bytes against the one-store form (u8 / 255 - mean) * (1 / std): a few fp32 roundings"""
    for name in tp.PREP_CASES:
        ref = torch.from_numpy(golden[name + ".image"])
        want = (ref.float() / 255 - torch.tensor(tp.MEAN).view(3, 1, 1)) / torch.tensor(tp.STD).view(3, 1, 1)
        got = tp.normalise(golden[name + ".image"])
        assert got.dtype == np.float32 and np.abs(got - want.numpy()).max() <= 4 * 2.0 ** -24 * 3.0


# ---- (c) mask, paddings, camera ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tp.PREP_CASES))
def test_prep_cases_against_context_crop(golden, name):
    from unidepth_amd import testprep
    img, mask, K, cons = tp.case_inputs(name)
    B, _, h, w = img.shape
    geo = testprep.test_geometry((h, w), tp.IMAGE_SHAPE, cons)
    assert geo.shape == tuple(golden[name + ".shape"]) and geo.window == tuple(golden[name + ".window"])
    assert geo.paddings == tuple(golden[name + ".paddings"]) and geo.zoom == float(golden[name + ".zoom"])
    r64 = tp.restate(img, geo.window, geo.shape, "bicubic", np.float64)
    bad, lvl, tie_bad, n_ex = compare_bytes(tp.restate(img, geo.window, geo.shape), r64, golden[name + ".image"])
    assert bad == 0 and lvl <= 1 and tie_bad == 0 and n_ex <= MAX_EXCLUDED * r64.size
    assert np.array_equal(tp.restate_mask(mask, (h, w), geo.window, geo.shape, B=B), golden[name + ".mask"])
    pl, pb, pr, pt = geo.paddings
    follows = h * w / (h + pb + pt) / (w + pl + pr) >= 0.5              # the reference leaves the camera alone below half valid area
    Kr = tp.restate_camera(K, geo.window, geo.shape[0]) if follows else K
    assert np.array_equal(Kr.view(np.int32), golden[name + ".K"].view(np.int32))
    assert follows == (name != "p60x300_wide")


# ---- (d) header and bindings ------------------------------------------------------------------------------------------------------

def test_resize_aa_descriptor_size_constants_and_package_exports():
    import unidepth_amd
    from unidepth_amd import _lib
    assert ctypes.sizeof(_lib.UdResizeAA) == 152
    for k, v in (("UD_RESIZE_BICUBIC", 0), ("UD_RESIZE_BILINEAR", 1), ("UD_RESIZE_OUT_F32", 0), ("UD_RESIZE_OUT_U8", 1),
                 ("UD_RESIZE_OUT_NORM", 2), ("UD_RESIZE_MAX_SCALE", 8), ("UD_RESIZE_MAX_TAPS", 33)):
        assert getattr(_lib, k) == v
    for name in ("TestGeometry", "test_geometry", "prepare_test_batch", "resize_aa", "original_image"):
        assert name in unidepth_amd.__all__ and callable(getattr(unidepth_amd, name))


def test_c_abi_refusals():
    """every refusal is made on the host before any launch (no GPU needed)"""
    from unidepth_amd import _lib

    def desc(**kw):
        d = _lib.UdResizeAA()
        d.src, d.dst = 4096, 8192
        d.B, d.C, d.h, d.w, d.top, d.left, d.height, d.width = 1, 3, 10, 10, 0, 0, 10, 10
        d.Ho, d.Wo, d.dtop, d.dleft, d.Hn, d.Wn = 5, 5, 0, 0, 5, 5
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, word in ((dict(src=None), "null"), (dict(B=0), "sizes"), (dict(Hn=0), "sizes"), (dict(B=30000), "sizes"),
                     (dict(height=41), "UD_RESIZE_MAX_SCALE"), (dict(width=10 * 8 + 1, Wo=10, Wn=10), "UD_RESIZE_MAX_SCALE"),
                     (dict(filter=2), "filter"), (dict(out_form=3), "out_form"), (dict(out_form=2, C=5), "C <= 4"),
                     (dict(dtop=1), "destination window"), (dict(dleft=-1), "destination window"), (dict(top=1 << 30), "window"),
                     (dict(src=4097), "aligned"), (dict(dst=8194), "aligned"), (dict(mask_src=64), "mask"), (dict(K_in=64), "K_in")):
        assert _lib.lib.ud_resize_aa(ctypes.byref(desc(**kw)), None) < 0, kw
        assert word in _lib.lib.ud_last_error().decode(), (kw, _lib.lib.ud_last_error())
    assert _lib.lib.ud_resize_aa(None, None) < 0


def test_argument_errors():
    from unidepth_amd import cameras, testprep
    cons = tp.CONSTRAINTS["small"]
    img = torch.zeros(1, 3, 20, 30, dtype=torch.uint8)
    kw = dict(image_shape=(518, 518), shape_constraints=cons)
    with pytest.raises(ValueError, match="hw"):
        testprep.test_geometry((0, 5), (518, 518), cons)
    with pytest.raises(ValueError, match="image_shape"):
        testprep.test_geometry((5, 5), (518,), cons)
    with pytest.raises(ValueError, match="shape_mult"):
        testprep.test_geometry((5, 5), (518, 518), {"ratio_bounds": [0.5, 2.5], "pixels_min": 1, "pixels_max": 2})
    with pytest.raises(ValueError, match="image"):
        testprep.prepare_test_batch(img.float(), **kw)
    with pytest.raises(ValueError, match="image"):
        testprep.prepare_test_batch(img[:, :2], **kw)
    with pytest.raises(ValueError, match="validity_mask"):
        testprep.prepare_test_batch(img, validity_mask=torch.zeros(1, 1, 20, 31, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="std"):
        testprep.prepare_test_batch(img, std=(1.0, 0.0, 1.0), **kw)
    with pytest.raises(ValueError, match="camera"):
        testprep.prepare_test_batch(img, camera=torch.eye(4), **kw)
    with pytest.raises(ValueError, match="camera"):
        testprep._camera_matrix(torch.eye(3).repeat(2, 1, 1), 3, "cpu")
    with pytest.raises(NotImplementedError, match="EUCM"):
        testprep._camera_matrix(cameras.EUCM(torch.tensor([10.0, 10.0, 5.0, 5.0, 0.5, 1.0])), 1, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        testprep.prepare_test_batch(img, **kw)                                   # CPU tensors are refused, not silently computed
    with pytest.raises(RuntimeError, match="GPU"):
        testprep.resize_aa(img, (14, 14))
    with pytest.raises(ValueError, match="mode"):
        testprep.resize_aa(img, (14, 14), mode="nearest")
    with pytest.raises(ValueError, match="size"):
        testprep.resize_aa(img, (14,))
    with pytest.raises(ValueError, match="size"):
        testprep.resize_aa(img, (0, 14))
    with pytest.raises(ValueError, match="window"):
        testprep.resize_aa(img, (14, 14), window=(0, 0, 0, 5))
    with pytest.raises(ValueError, match="x must"):
        testprep.resize_aa(img[0], (14, 14))
    with pytest.raises(ValueError, match="x must"):
        testprep.resize_aa(img.int(), (14, 14))
    with pytest.raises(ValueError, match="out_dtype"):
        testprep.resize_aa(img, (14, 14), out_dtype=torch.int32)
    with pytest.raises(ValueError, match="more than 8"):
        testprep.resize_aa(torch.zeros(1, 1, 113, 10), (14, 10))
    with pytest.raises(ValueError, match="virtual_size"):
        testprep.resize_aa(img, (14, 14), virtual_size=(20, 20), origin=(7, 0))
    with pytest.raises(ValueError, match="batch"):
        testprep.original_image({"data": {}})
    data = {"image": torch.zeros(2, 3, 14, 14), "depth": torch.zeros(2, 1, 20, 20)}
    with pytest.raises(ValueError, match="one padding"):
        testprep.original_image({"data": dict(data), "img_metas": [{"paddings": [0, 1, 0, 1]}, {"paddings": [0, 2, 0, 1]}]})
    with pytest.raises(ValueError, match="paddings"):
        testprep.original_image({"data": dict(data), "img_metas": [{"paddings": [0, -1, 0, 1]}]})


# ---- (e) planted defects ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("defect", ["unnormalised", "plain_support", "image_extent", "half_up"])
def test_planted_defects_are_caught(golden, defect):
    """the comparison of (b) applied to a restatement with one defect: weights left unnormalised, the support not scaled on
    down-sampling (plain bicubic / bilinear), `in` taken from the image instead of the window, round-half-up"""
    caught = []
    for name in tp.WINDOW_CASES:
        u8, _, win, size = tp.case_inputs(name)
        for filt in tp.FILTERS:
            r64 = tp.restate(u8, win, size, filt, np.float64)
            r32 = tp.restate(u8, win, size, filt, np.float32, defect=defect)
            dev = float(np.nan_to_num(np.abs(r32 - r64), nan=np.inf).max())
            bad, lvl, tie_bad, _ = compare_bytes(r32, r64, golden[f"{name}.{filt}.u8"], defect)
            if dev > TOL_U8 or bad or lvl > 1 or tie_bad:
                caught.append((name, filt))
    print(defect, "caught on", caught)
    need = {"unnormalised": ("w97x131_cut", "bicubic"), "plain_support": ("w97x131_cut", "bilinear"),
            "image_extent": ("w45x60_pad_lr", "bicubic"), "half_up": ("w9x11_full", "bilinear")}[defect]
    assert need in caught
