"""GPU tests of ud_resize_aa (csrc/testprep.hip, unidepth_amd/testprep.py) against the numpy fp32 restatement of
tools/make_golden_testprep.py (pinned to the reference's own arrays by tests/test_testprep_cpu.py): every destination sits inside a
sentinel-filled guard allocation (tests/layout_guard.py for fp32; a byte guard of the same kind here for uint8), results are compared
bit for bit, guards must be intact.  The shapes are the kernel's seams, not the workload's: destination rows that start 0..3 elements
past a vector boundary, more than one tile along both axes, windows that pad, cut or miss the image, one-row and one-column sources,
identity, up-scaling, the largest supported down-scaling (33 taps, several staging chunks) and source rows off their 16-byte
boundary."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import layout_guard as lg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_testprep", os.path.join(ROOT, "tools", "make_golden_testprep.py"))
tp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tp)

BYTE_SENTINEL = 0xBD
FORMS = ("f32", "u8", "norm")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class ByteGuard:
    """`n` uint8 elements starting `off` bytes past a 256-byte boundary inside an allocation filled with BYTE_SENTINEL"""

    def __init__(self, n, off):
        self.buf = torch.full((512 + n + 512,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.hi = 256 + off, 256 + off + n
        self.view = self.buf[self.lo:self.hi]

    def check_guards(self, name="output"):
        bad = self.buf != BYTE_SENTINEL
        bad[self.lo:self.hi] = False
        n = int(bad.sum())
        assert n == 0, f"{name}: {n} guard byte(s) rewritten; first at {int(bad.nonzero()[0]) - self.lo} (view-relative)"


def _device_src(arr, off):
    """arr on the device, its first element `off` elements past a 256-byte boundary (rows off their 16-byte boundary)"""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_same(got, ref, what):
    if not np.array_equal(_bits(got), _bits(ref)):
        bad = np.argwhere(_bits(got) != _bits(ref))
        raise AssertionError(f"{what}: {len(bad)} element(s) differ from the fp32 restatement; first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} vs {ref[tuple(bad[0])]!r}")


def _run(src, window, size, filt, form, off=0, src_off=0, mask="none", K=None, virtual=None, origin=(0, 0)):
    """One ud_resize_aa on guarded destinations (image rows start `off` elements past a 16-byte boundary at row 0, the mask plane
    off + 1), compared bitwise with the restatement.  mask: "none", "ones" (implied) or a uint8 array [B,1,h,w]."""
    from unidepth_amd import _lib, testprep
    B, Cn, h, w = src.shape
    Hn, Wn = size
    window = tuple(window) if window is not None else (0, 0, h, w)
    n = B * Cn * Hn * Wn
    s = _device_src(src, src_off)
    guards = []
    if form == "u8":
        g = ByteGuard(n, off)
        dst = g.view.view(B, Cn, Hn, Wn)
    else:
        g = lg.guarded(1, n, (n + 131) // 4 * 4, torch.float32, pre_rows=1, post_rows=1, offset_cols=32 + off)
        dst = g.view.view(B, Cn, Hn, Wn)
    guards.append(g)
    m_src = m_dst = None
    has_mask = not (isinstance(mask, str) and mask == "none")
    if has_mask:
        gm = ByteGuard(B * Hn * Wn, off + 1)
        m_dst = gm.view.view(B, 1, Hn, Wn)
        m_src = None if isinstance(mask, str) else _device_src(mask, src_off)
        guards.append(gm)
    Kin = Kout = None
    if K is not None:
        Kin = torch.from_numpy(K).cuda()
        gk = lg.guarded(1, B * 9, B * 9 + 64, torch.float32, pre_rows=1, post_rows=1, offset_cols=17)
        Kout = gk.view
        guards.append(gk)
    mean = np.asarray(tp.MEAN + (0.5,), dtype=np.float32)[:Cn]
    inv_std = (np.float32(1) / np.asarray(tp.STD + (0.25,), dtype=np.float32))[:Cn]
    testprep.launch(s, dst, window, _lib.UD_RESIZE_BICUBIC if filt == "bicubic" else _lib.UD_RESIZE_BILINEAR,
                    {"f32": _lib.UD_RESIZE_OUT_F32, "u8": _lib.UD_RESIZE_OUT_U8, "norm": _lib.UD_RESIZE_OUT_NORM}[form],
                    virtual=virtual, origin=origin, mask_src=m_src, mask_dst=m_dst, K_in=Kin, K_out=Kout,
                    mean=mean.tolist(), inv_std=inv_std.tolist())
    torch.cuda.synchronize()
    v = tp.restate(src, window, size, filt, np.float32, virtual=virtual, origin=origin)
    if form == "f32":
        ref = v
    elif form == "u8":
        ref = tp.to_u8(v)
    else:
        ref = (((tp.to_u8(v).astype(np.float32) / np.float32(255)).astype(np.float32) - mean.reshape(-1, 1, 1)).astype(np.float32)
               * inv_std.reshape(-1, 1, 1)).astype(np.float32)
    _assert_same(dst.cpu().numpy(), ref, f"{form} image")
    if has_mask:
        refm = tp.restate_mask(None if isinstance(mask, str) else mask, (h, w), window, size, B=B, virtual=virtual, origin=origin)
        _assert_same(m_dst.cpu().numpy(), refm, "mask plane")
    if K is not None:
        _assert_same(Kout.cpu().numpy().reshape(B, 3, 3), tp.restate_camera(K, window, (virtual or size)[0]), "intrinsics")
    for i, g in enumerate(guards):
        g.check_guards(f"output {i}")
    return dst


def _rnd_u8(rng, *shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _rnd_f32(rng, *shape):
    return (rng.random(shape, dtype=np.float32) * np.float32(384) - np.float32(64)).astype(np.float32)


# ---- the C-ABI on the seams -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("filt", tp.FILTERS)
@pytest.mark.parametrize("name", list(tp.WINDOW_CASES))
def test_windows_bitwise_and_guards(name, filt, B):
    """the seven windows: both source dtypes, the three output forms, the mask plane (given / implied) and the intrinsics; the
    destination offset and the source offset walk through 0..3 elements"""
    (h, w), win, size = tp.WINDOW_CASES[name]
    rng = np.random.default_rng(100 * B + h + (filt == "bilinear"))
    k = 0
    for src in (_rnd_u8(rng, B, 3, h, w), _rnd_f32(rng, B, 3, h, w)):
        for form in FORMS:
            mask = ("none", "ones", _rnd_u8(rng, B, 1, h, w) % 3)[k % 3]
            K = _rnd_f32(rng, B, 3, 3) if k % 2 else None
            _run(src, win, size, filt, form, off=k % 4, src_off=(k + B) % 4, mask=mask, K=K)
            k += 1


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("Wn", [14, 28, 42, 70])
def test_destination_rows_off_their_boundary(Wn, off):
    """rows of 14, 28, 42 and 70 pixels whose first one starts 0..3 elements past a 16-byte (fp32) / 4-byte (uint8) boundary: scalar
    head, vector body, tail; 70 pixels + 3 need two tiles"""
    rng = np.random.default_rng(Wn * 4 + off)
    src = _rnd_u8(rng, 2, 2, 23, 57)
    for form, filt in (("f32", "bicubic"), ("u8", "bilinear"), ("norm", "bicubic")):
        _run(src, (-2, -3, 27, 62), (9, Wn), filt, form, off=off, src_off=off, mask="ones")


@pytest.mark.parametrize("filt", tp.FILTERS)
def test_one_row_one_column_and_beside(filt):
    rng = np.random.default_rng(5)
    _run(_rnd_f32(rng, 1, 2, 1, 40), None, (14, 28), filt, "f32", off=1)                        # a one-row source
    _run(_rnd_u8(rng, 2, 1, 40, 1), None, (28, 14), filt, "u8", off=3, mask="ones")             # a one-column source
    _run(_rnd_u8(rng, 1, 3, 1, 1), (-1, -1, 3, 3), (14, 14), filt, "norm", off=2)
    for win in ((0, 25, 20, 30), (-40, 0, 20, 25), (30, -10, 12, 9)):                           # beside / above / below the image
        dst = _run(_rnd_u8(rng, 1, 3, 20, 25) | 1, win, (14, 28), filt, "f32", off=1, mask=_rnd_u8(rng, 1, 1, 20, 25) | 1)
        assert not bool(dst.any())


@pytest.mark.parametrize("filt", tp.FILTERS)
def test_identity_is_a_bit_copy(filt):
    rng = np.random.default_rng(7)
    src = _rnd_f32(rng, 2, 2, 21, 67)
    src[0, 0, 3, 4], src[0, 1, 5, 6], src[1, 0, 7, 8] = -0.0, np.inf, -np.inf
    dst = _run(src, None, (21, 67), filt, "f32", off=1, src_off=3)
    assert np.array_equal(dst.cpu().numpy().view(np.int32), src.view(np.int32))
    dst = _run(src, (2, 3, 16, 50), (16, 50), filt, "f32", off=2)                                # a window at its own size: a crop
    assert np.array_equal(dst.cpu().numpy().view(np.int32), np.ascontiguousarray(src[:, :, 2:18, 3:53]).view(np.int32))
    u8 = _rnd_u8(rng, 1, 3, 15, 22)
    dst = _run(u8, None, (15, 22), filt, "u8", off=3, src_off=1)
    assert np.array_equal(dst.cpu().numpy(), u8)
    fin = _rnd_f32(rng, 2, 2, 21, 67)                                                            # one axis copied, the other resized
    _run(fin, None, (21, 30), filt, "f32")
    _run(fin, None, (40, 67), filt, "f32")


@pytest.mark.parametrize("filt", tp.FILTERS)
def test_largest_downscale_upscale_and_many_tiles(filt):
    """scale 8 (the documented bound: 33 bicubic taps, 4 rows per staging chunk), 7.x with odd sizes, a 12-fold up-scale, and
    destinations of several tiles along both axes"""
    rng = np.random.default_rng(11)
    _run(_rnd_u8(rng, 1, 1, 112, 1120), None, (14, 140), filt, "f32", off=1, src_off=1)
    _run(_rnd_u8(rng, 1, 2, 101, 555), (-3, -7, 109, 570), (14, 72), filt, "u8", off=2, src_off=3, mask="ones")
    _run(_rnd_f32(rng, 1, 1, 5, 7), None, (60, 84), filt, "f32", off=3)
    _run(_rnd_u8(rng, 2, 3, 60, 200), (-4, 3, 70, 190), (23, 135), filt, "norm", off=1, src_off=2, mask=_rnd_u8(rng, 2, 1, 60, 200) % 2,
         K=_rnd_f32(rng, 2, 3, 3))


def test_beyond_the_bound_is_refused():
    from unidepth_amd import _lib, testprep
    src = torch.zeros(1, 1, 113, 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty(1, 1, 14, 20, device="cuda")
    with pytest.raises(RuntimeError, match="UD_RESIZE_MAX_SCALE"):
        testprep.launch(src, dst, (0, 0, 113, 20), _lib.UD_RESIZE_BICUBIC, _lib.UD_RESIZE_OUT_F32)
    with pytest.raises(ValueError, match="more than 8"):
        testprep.resize_aa(src, (14, 20))


def test_destination_window_of_a_larger_resize():
    """virtual size + origin: the pixels of a full resize followed by a crop, bit for bit"""
    rng = np.random.default_rng(13)
    src = _rnd_f32(rng, 2, 1, 28, 42)
    full = tp.restate(src, None, (45, 71), "bilinear")
    dst = _run(src, None, (37, 53), "bilinear", "f32", off=1, virtual=(45, 71), origin=(5, 11), mask="ones")
    assert np.array_equal(dst.cpu().numpy().view(np.int32), np.ascontiguousarray(full[:, :, 5:42, 11:64]).view(np.int32))


# ---- the Python surface --------------------------------------------------------------------------------------------------------------

def _prep(name, **kw):
    from unidepth_amd import prepare_test_batch
    img, mask, K, cons = tp.case_inputs(name)
    inputs, metas = prepare_test_batch(torch.from_numpy(img).cuda(), camera=torch.from_numpy(K).cuda(),
                                       validity_mask=None if mask is None else torch.from_numpy(mask).cuda(),
                                       image_shape=tp.IMAGE_SHAPE, shape_constraints=cons, **kw)
    return img, mask, K, cons, inputs, metas


@pytest.mark.parametrize("name", list(tp.PREP_CASES))
def test_prepare_test_batch_on_golden_cases(name):
    """bit-equal to the restatement; against the reference's ContextCrop output under the conditions of the CPU test: bytes equal
    outside the 4e-3 band around half-integers, within one level inside it, at most 3 % excluded; mask, paddings, camera equal"""
    from unidepth_amd import testprep
    g = np.load(tp.GOLDEN)
    img, mask, K, cons, inputs, metas = _prep(name)
    B, _, h, w = img.shape
    geo = testprep.test_geometry((h, w), tp.IMAGE_SHAPE, cons)
    assert list(inputs) == ["image", "validity_mask", "camera"] and len(metas) == B
    assert inputs["image"].dtype == torch.float32 and tuple(inputs["image"].shape) == (B, 3) + geo.shape
    u = tp.to_u8(tp.restate(img, geo.window, geo.shape))
    _assert_same(inputs["image"].cpu().numpy(), tp.normalise(u), "normalised image")
    r64 = tp.restate(img, geo.window, geo.shape, "bicubic", np.float64)
    ex = np.abs(r64 - np.floor(r64) - 0.5) <= 4e-3
    ref = g[name + ".image"]
    assert not ((u != ref) & ~ex).any() and np.abs(u.astype(int) - ref).max() <= 1 and ex.mean() <= 0.03
    # the float image the reference feeds its network: /255 and TF.normalize of its own bytes
    want = (torch.from_numpy(ref).float() / 255 - torch.tensor(tp.MEAN).view(3, 1, 1)) / torch.tensor(tp.STD).view(3, 1, 1)
    same = torch.from_numpy(u == ref)
    assert float(((inputs["image"].cpu() - want).abs() * same).max()) <= 4 * 2.0 ** -24 * 3.0
    assert np.array_equal(inputs["validity_mask"].cpu().numpy(), g[name + ".mask"])
    _assert_same(inputs["camera"].cpu().numpy(), g[name + ".K"], "camera")
    for m in metas:
        assert list(m["paddings"]) == list(g[name + ".paddings"]) and m["image_rescale"] == float(g[name + ".zoom"])
        assert list(m["resized_shape"]) == list(g[name + ".shape"])


def test_prepare_test_batch_camera_forms_and_depth():
    from unidepth_amd import cameras, prepare_test_batch
    img, _, K, cons = tp.case_inputs("p37x53")
    t = torch.from_numpy(img).cuda()
    kw = dict(image_shape=tp.IMAGE_SHAPE, shape_constraints=cons)
    depth = torch.zeros(2, 1, 37, 53, device="cuda")
    a, _ = prepare_test_batch(t, depth, torch.from_numpy(K[0]), **kw)                            # one CPU [3,3] matrix for the batch
    b, _ = prepare_test_batch(t, camera=cameras.Pinhole(K=torch.from_numpy(K[:1])), **kw)
    c, _ = prepare_test_batch(t, validity_mask=torch.ones(2, 1, 37, 53, dtype=torch.bool, device="cuda"), **kw)
    assert a["depth"] is depth and "depth" not in b and "camera" not in c
    ref = tp.restate_camera(np.repeat(K[:1], 2, axis=0), (-2, 0, 40, 53), 42)
    _assert_same(a["camera"].cpu().numpy(), ref, "camera")
    _assert_same(b["camera"].cpu().numpy(), ref, "camera")
    assert torch.equal(a["validity_mask"], c["validity_mask"]) and torch.equal(a["image"], b["image"])
    with pytest.raises(NotImplementedError, match="EUCM"):
        prepare_test_batch(t, camera=cameras.EUCM(torch.tensor([10.0, 10.0, 5.0, 5.0, 0.5, 1.0])), **kw)


@pytest.mark.parametrize("mode", tp.FILTERS)
def test_resize_aa_is_interpolate_antialias(mode):
    """the drop-in: bit-equal to the restatement, and within the CPU test's tolerance of F.interpolate(antialias=True) on this GPU"""
    import torch.nn.functional as F
    from unidepth_amd import resize_aa
    u8, f32, win, size = tp.case_inputs("w45x60_pad_lr")
    x = torch.from_numpy(f32).cuda()
    out = resize_aa(x, size, mode)
    assert out.dtype == torch.float32
    _assert_same(out.cpu().numpy(), tp.restate(f32, None, size, mode), "resize_aa")
    lib = F.interpolate(x, size=size, mode=mode, antialias=True, align_corners=False)
    assert float((out - lib).abs().max()) <= 4 * 1.52e-3
    o8 = resize_aa(torch.from_numpy(u8).cuda(), size, mode, window=win)
    assert o8.dtype == torch.uint8
    _assert_same(o8.cpu().numpy(), tp.to_u8(tp.restate(u8, win, size, mode)), "resize_aa uint8")
    of = resize_aa(torch.from_numpy(u8).cuda(), size, mode, window=win, out_dtype=torch.float32)
    _assert_same(of.cpu().numpy(), tp.restate(u8, win, size, mode), "resize_aa uint8 -> fp32")
    comp = tp.torch_composition(torch.from_numpy(u8).cuda(), win, size, mode, out="f32")
    assert float((of - comp).abs().max()) <= 4 * 1.05e-3
    half = resize_aa(x.half(), size, mode)
    assert half.dtype == torch.float16
    assert torch.equal(half.cpu(), torch.from_numpy(tp.restate(x.half().float().cpu().numpy(), None, size, mode)).half())


def test_original_image_round_trip():
    """prepare_test_batch, then original_image back at the ground truth's size: shapes, and bits against the restatement"""
    from unidepth_amd import original_image, testprep
    img, mask, K, cons, inputs, metas = _prep("p97x131")
    h, w = img.shape[-2:]
    geo = testprep.test_geometry((h, w), tp.IMAGE_SHAPE, cons)
    Hn, Wn = geo.shape
    g = torch.Generator().manual_seed(3)
    pred = (1.0 + 5.0 * torch.rand(1, 1, Hn, Wn, generator=g)).cuda()
    net = inputs["image"].clone()
    batch = {"data": {"image": inputs["image"], "depth": torch.zeros(1, 1, h, w, device="cuda")}, "img_metas": metas}
    batch2, preds = original_image(batch, {"depth": pred.clone(), "other": 1})
    assert batch2 is batch and tuple(batch["data"]["image"].shape) == (1, 3, h, w) and tuple(preds["depth"].shape) == (1, 1, h, w)
    left, top, right, bottom = metas[0]["paddings"]
    virt, org = (h + top + bottom, w + left + right), (top, left)
    _assert_same(batch["data"]["image"].cpu().numpy(), tp.restate(net.cpu().numpy(), None, (h, w), "bilinear", virtual=virt, origin=org), "image")
    _assert_same(preds["depth"].cpu().numpy(), tp.restate(pred.cpu().numpy(), None, (h, w), "bilinear", virtual=virt, origin=org), "depth")
    assert preds["other"] == 1
    # zero paddings: the plain antialiased resize to the ground truth's size
    b0 = {"data": {"image": net, "depth": torch.zeros(1, 1, 50, 61, device="cuda")}, "img_metas": [{}]}
    original_image(b0)
    _assert_same(b0["data"]["image"].cpu().numpy(), tp.restate(net.cpu().numpy(), None, (50, 61), "bilinear"), "image, no paddings")


def test_calls_are_reproducible():
    a = _prep("p120x41_tall")[4]
    b = _prep("p120x41_tall")[4]
    for k in ("image", "validity_mask", "camera"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_prepare_then_forward_test_vits():
    """raw uint8 images -> prepare_test_batch -> model(inputs, metas) on a seeded ViT-S checkpoint equals forward_test fed with the
    restatement's arrays, bit for bit; depth comes back at the ground truth's size"""
    from oracle import synth
    from unidepth_amd import UniDepthV2, prepare_test_batch, testprep
    cfg = synth.load_config("vits14")
    model = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, 123)).to("cuda").eval()
    cons = dict(ratio_bounds=[0.5, 2.5], pixels_max=30000, pixels_min=20000, shape_mult=14, sample=True)
    B, h, w = 2, 90, 161
    g = torch.Generator().manual_seed(17)
    img = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    K = torch.tensor([[[150.0, 0.0, 80.0], [0.0, 151.0, 44.5], [0.0, 0.0, 1.0]]]).repeat(B, 1, 1)
    depth = torch.zeros(B, 1, h, w, device="cuda")
    geo = testprep.test_geometry((h, w), tp.IMAGE_SHAPE, cons)
    inputs, metas = prepare_test_batch(img.cuda(), depth, K, image_shape=tp.IMAGE_SHAPE, shape_constraints=cons)
    out = model(inputs, metas)
    ref_in = {"image": torch.from_numpy(tp.normalise(tp.to_u8(tp.restate(img.numpy(), geo.window, geo.shape)))).cuda(), "depth": depth,
              "camera": torch.from_numpy(tp.restate_camera(K.numpy(), geo.window, geo.shape[0])).cuda()}
    ref = model.forward_test(ref_in, [{"paddings": list(geo.paddings)} for _ in range(B)])
    torch.cuda.synchronize()
    assert tuple(out["depth"].shape) == (B, 1, h, w) and bool(torch.isfinite(out["depth"]).all())
    for k in ref:
        assert torch.equal(out[k].contiguous().view(torch.int32), ref[k].contiguous().view(torch.int32)), k
