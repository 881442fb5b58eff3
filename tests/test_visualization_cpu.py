"""Colourising without a GPU (unidepth_amd/visualization.py, include/unidepth_hip.h UdColorize): the numpy restatement of
tools/make_golden_colorize.py and the host colorize / image_grid against the reference's own bytes (tests/golden/colorize.npz), the
generated colormap tables, save_png, the C-ABI's refusals and workspace query, and the Python argument errors."""
import ctypes as C
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_colorize", os.path.join(ROOT, "tools", "make_golden_colorize.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

CHUNK = 1024         # csrc/colorize.hip CZ_CHUNK


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(mg.GOLDEN))


def _dtype(v):
    return np.float64 if v.dtype == np.float64 else np.float32


def test_golden_has_every_case(golden):
    luts = {"lut_" + c[5] for c in mg.CASES.values()}
    assert sorted(golden) == sorted(set(mg.CASES) | set(mg.GRIDS) | luts)
    assert {"lut_magma_r", "lut_coolwarm"} <= luts
    for name, (_, H, W, _, _, _) in mg.CASES.items():
        assert golden[name].dtype == np.uint8 and golden[name].shape == (H, W, 3), name
    assert os.path.getsize(mg.GOLDEN) < 200 * 1024
    # what the cases must cover: both / one / no limit on two colormaps, float64, bin edges, the invalid threshold, NaN, inf, a constant
    for cmap in ("magma_r", "coolwarm"):
        limits = {(c[3] is None, c[4] is None) for c in mg.CASES.values() if c[5] == cmap}
        assert limits == {(False, False), (True, False), (False, True), (True, True)}
    assert mg.case_inputs("f64_both_magma_r").dtype == np.float64
    sp = mg.case_inputs("special_magma_r").reshape(-1)
    assert sp.dtype == np.float32 and np.float32(1e-4) in sp and mg.BELOW_INVALID in sp and mg.BELOW_INVALID < np.float32(1e-4)
    assert np.isnan(sp).any() and np.inf in sp and -np.inf in sp and np.float32(10.0) in sp and (sp > 10.0).any() and (sp < 0.01).any()
    assert np.isnan(mg.case_inputs("nan_auto")).sum() == 1 and not golden["nan_auto"].any()              # whole image black
    assert np.unique(mg.case_inputs("const_auto")).size == 1
    e = mg.case_inputs("edges_magma_r")
    assert np.array_equal(e[0], (0.01 + (10.0 - 0.01) * np.arange(257) / 256.0).astype(np.float32))


@pytest.mark.parametrize("name", list(mg.CASES))
def test_restatement_matches_reference_golden(name, golden):
    _, _, _, vmin, vmax, cmap = mg.CASES[name]
    v = mg.case_inputs(name)
    got = mg.restate(v, golden["lut_" + cmap], vmin, vmax, dtype=_dtype(v))
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, golden[name])


@pytest.mark.parametrize("name", list(mg.CASES))
def test_host_colorize_matches_reference_golden(name, golden):
    from unidepth_amd import colorize
    _, _, _, vmin, vmax, cmap = mg.CASES[name]
    v = mg.case_inputs(name)
    before = v.copy()
    got = colorize(v, vmin=vmin, vmax=vmax, cmap=cmap)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, golden[name])
    assert np.array_equal(v, before, equal_nan=True)                       # the input is not modified
    np.testing.assert_array_equal(colorize(v[..., None], vmin, vmax, cmap), golden[name])      # [H,W,1] is squeezed


def test_error_map_case_is_the_fp32_error_of_its_inputs():
    g, p = mg.arel_inputs()
    e = mg.case_inputs("arel_coolwarm")
    assert e.dtype == np.float32 and (g == 0).sum() > 10 and (e[g == 0] == 0).all() and e[3, 4] == 0.0
    with np.errstate(all="ignore"):
        want = np.abs(g.astype(np.float64) - p) / g
    ok = g != 0
    assert np.abs(e[ok] - want[ok]).max() <= 2.0 ** -22 * want[ok].max()


def test_host_colorize_passes_rgb_through_and_defaults():
    from unidepth_amd import colorize
    rgb = mg.case_rgb()
    assert colorize(rgb) is rgb
    v = mg.case_inputs("none_magma_r")
    np.testing.assert_array_equal(colorize(v), colorize(v, None, None, "magma_r"))
    with pytest.raises(ValueError, match="known: .*magma_r"):
        colorize(v, cmap="no_such_map")


def test_generated_tables(golden):
    from unidepth_amd import colormaps
    want = [n + s for n in ("magma", "inferno", "plasma", "viridis", "turbo", "coolwarm", "gray", "Spectral") for s in ("", "_r")]
    assert set(want) <= set(colormaps.NAMES)
    for name in colormaps.NAMES:
        t = colormaps.get_table(name)
        assert t.dtype == np.uint8 and t.shape == (256, 3) and not t.flags.writeable
    for key in golden:
        if key.startswith("lut_"):
            np.testing.assert_array_equal(colormaps.get_table(key[4:]), golden[key])
    g = colormaps.get_table("gray")
    assert g[0].tolist() == [0, 0, 0] and g[255].tolist() == [255, 255, 255] and (g[:, 0] == g[:, 1]).all() and (np.diff(g[:, 0].astype(int)) >= 0).all()
    # a reversed segment-data map is stored, never derived: its bytes need not be the flip of its base (gray_r is not)
    r = colormaps.get_table("gray_r")
    assert r[0].tolist() == [255, 255, 255] and r[255].tolist() == [0, 0, 0] and np.abs(r.astype(int) - g[::-1].astype(int)).max() <= 1
    assert np.array_equal(colormaps.get_table("magma_r"), colormaps.get_table("magma")[::-1])         # a listed map reverses exactly
    with open(os.path.join(ROOT, "unidepth_amd", "colormaps.py")) as f:
        src = f.read()
    assert "import matplotlib" not in src and "GENERATED" in src
    with open(os.path.join(ROOT, "unidepth_amd", "visualization.py")) as f:
        assert "import matplotlib" not in f.read()


@pytest.mark.parametrize("name", list(mg.GRIDS))
def test_image_grid_matches_reference_golden(name, golden):
    from unidepth_amd import image_grid
    rows, cols, cells = mg.GRIDS[name]
    imgs = [mg.case_rgb() if c == "rgb" else golden[c] for c in cells]
    np.testing.assert_array_equal(image_grid(imgs, rows, cols), golden[name])
    np.testing.assert_array_equal(mg.restate_grid(imgs, rows, cols), golden[name])


def test_image_grid_edges():
    from unidepth_amd import image_grid
    assert image_grid([], 2, 2) is None
    a = np.full((4, 6, 3), 7, np.uint8)
    with pytest.raises(ValueError):
        image_grid([a, a, a], 2, 2)
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(ValueError, match="PIL"):
            image_grid([a, np.zeros((8, 12, 3), np.uint8)], 1, 2)
    else:
        g = image_grid([a, np.full((8, 12, 3), 9, np.uint8)], 1, 2)
        assert g.shape == (4, 12, 3) and (g[:, :6] == 7).all() and (g[:, 6:] == 9).all()


def _parse_png(raw):
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        pos += 12 + n
    return chunks


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (24, 31)])
def test_save_png_roundtrip(tmp_path, H, W):
    from unidepth_amd import save_png
    img = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    path = tmp_path / "a.png"
    save_png(str(path), torch.from_numpy(img) if H == 5 else img)
    chunks = _parse_png(path.read_bytes())
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(H, W, 3), img)
    for bad in (img.astype(np.float32), img[..., 0], img[..., :2]):
        with pytest.raises(ValueError):
            save_png(str(tmp_path / "b.png"), bad)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------

def test_colorize_rejects_bad_descriptors_without_a_launch():
    """every refusal comes back before any HIP call: this runs on a machine without a GPU, the pointers are never followed"""
    from unidepth_amd import _lib
    lib = _lib.lib
    P = 0x1000                                      # stands for a device pointer
    B, H, W = 2, 5, 7
    nbytes = lib.ud_colorize_work_bytes(B, H, W)

    def rc(panel=None, panels=None, **kw):
        d = _lib.UdColorize()
        base = dict(dst=P, work=P, work_bytes=nbytes, B=B, H=H, W=W, rows=1, cols=1, flags=0)
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        for i, spec in enumerate(panels if panels is not None else [panel or {}]):
            p = dict(kind=_lib.UD_CZ_MAP, src=P, lut=P, batch_stride=H * W, den=1.0)
            p.update(spec)
            for k, v in p.items():
                setattr(d.panels[i], k, v)
        r = lib.ud_colorize(C.byref(d), None)
        return r, lib.ud_last_error().decode()

    r, msg = lib.ud_colorize(None, None), lib.ud_last_error().decode()
    assert r < 0 and "null descriptor" in msg
    arel = dict(kind=_lib.UD_CZ_AREL, src2=P, batch_stride2=H * W)
    for kw, word in ((dict(dst=None), "null pointer (dst)"),
                     (dict(panel=dict(src=None)), "null pointer (src"),
                     (dict(panel=dict(lut=None)), "null pointer (src"),
                     (dict(panel=dict(arel, src2=None)), "null pointer (src"),
                     (dict(panel=dict(kind=_lib.UD_CZ_RGB, src=None)), "null pointer (src"),
                     (dict(rows=2, cols=3), "bad grid"), (dict(rows=5, cols=1), "bad grid"), (dict(rows=1, cols=5), "bad grid"),
                     (dict(rows=0), "bad grid"), (dict(cols=-1), "bad grid"), (dict(rows=65536, cols=65536), "bad grid"),
                     (dict(B=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-1), "bad sizes"), (dict(B=65536), "bad sizes"),
                     (dict(H=65536, W=65536), "bad sizes"),
                     (dict(H=0x7fffffff, W=1), "bad sizes"), (dict(H=1 << 26, W=1), "bad sizes"),   # thin and tall: the launch's x extent
                     (dict(H=(1 << 26) - 3, W=31), "bad sizes"),                                     # H*W < 2^31, one tile too many
                     (dict(H=1, W=400000000, cols=2, rows=1, panels=[{}, {}]), "bad sizes"),        # 3 * cols * W >= 2^31
                     (dict(flags=2), "unknown flag"),
                     (dict(panel=dict(kind=4)), "bad panel"), (dict(panel=dict(kind=-1)), "bad panel"), (dict(panel=dict(flags=4)), "bad panel"),
                     (dict(panel=dict(batch_stride=-1)), "batch_stride"),
                     (dict(panel=dict(arel, batch_stride2=-1)), "batch_stride"),
                     (dict(panel=dict(src=P + 2)), "4-byte aligned"),
                     (dict(panel=dict(arel, src2=P + 1)), "4-byte aligned"),
                     (dict(panel=dict(kind=_lib.UD_CZ_NONE)), "nothing to do"),
                     (dict(panel=dict(flags=_lib.UD_CZ_AUTO_LO), work=None), "null pointer (work"),
                     (dict(panel=dict(flags=_lib.UD_CZ_AUTO_HI), work=P + 2), "work not 4-byte aligned"),
                     (dict(panel=dict(flags=3), work_bytes=nbytes - 1), "workspace smaller"),
                     (dict(rows=2, cols=2, panels=[{}, {}, {}, dict(flags=1)], work_bytes=0), "workspace smaller")):
        r, msg = rc(**kw)
        assert r < 0 and word in msg, (kw, r, msg)


def test_work_bytes():
    from unidepth_amd import _lib
    wb = _lib.lib.ud_colorize_work_bytes
    for B, H, W in ((1, 1, 1), (1, 32, 32), (3, 37, 53), (8, 518, 518), (8, 480, 640)):
        n = wb(B, H, W)
        assert n == B * 4 * -(-H * W // CHUNK) * 12              # (min, max, has-NaN) per panel slot and chunk
        assert wb(B + 1, H, W) > n and wb(B, H + CHUNK, W) > n and wb(B, H, W + CHUNK) > n
    assert wb(0, 4, 4) < 0 and wb(1, 0, 4) < 0 and wb(1, 4, -1) < 0 and wb(1, 65536, 65536) < 0 and wb(65536, 4, 4) < 0
    # the render launch takes at most 2^24 - 1 tiles of 4 rows x 256 pixels (include/unidepth_hip.h UD_COLORIZE_MAX_TILES)
    assert wb(1, (1 << 26) - 4, 1) > 0 and wb(1, (1 << 26) - 3, 1) < 0 and wb(1, (1 << 26) - 4, 31) > 0 and wb(1, (1 << 26) - 3, 31) < 0


# ---- Python argument errors (CPU tensors: every check comes before any launch) -------------------------------------------------------

def test_argument_errors():
    from unidepth_amd import colorize, colorize_batch, demo_panel
    m = torch.ones(2, 6, 8)
    rgb = torch.zeros(2, 3, 6, 8, dtype=torch.uint8)
    for kw in (dict(maps=m.double()), dict(maps=torch.ones(6, 8)), dict(maps=torch.ones(2, 2, 6, 8)), dict(maps=m.numpy()),
               dict(maps=torch.ones(0, 6, 8)), dict(maps=m, vmin="low"), dict(maps=m, cmap="no_such_map"),
               dict(maps=m)):                                              # a CPU tensor: there is no CPU path for tensors
        with pytest.raises(ValueError):
            colorize_batch(**kw)
    with pytest.raises(ValueError, match="no CPU path"):
        colorize_batch(m)
    with pytest.raises(ValueError, match="no CPU path"):
        colorize(m, 0.0, 1.0)
    for t in (torch.ones(2, 2, 6, 8), torch.ones(1, 1, 1, 6, 8), torch.ones(8)):
        with pytest.raises(ValueError):
            colorize(t)
    for args, kw in (((rgb.float(), m), {}), ((rgb[:, :2], m), {}), ((rgb, m[:, :5]), {}), ((rgb, m.double()), {}), ((rgb, m, m[:1]), {}),
                     ((rgb, m), dict(depth_range=5.0)), ((rgb, m), dict(error_range=(0.0, 1.0, 2.0))), ((rgb, m), dict(cmap="nope")),
                     ((rgb, m, m), dict(error_cmap="nope")), ((rgb, m), dict(depth_range=("a", 1.0))),
                     ((rgb, m), {}), ((rgb, m, m), {})):                    # CPU tensors
        with pytest.raises(ValueError):
            demo_panel(*args, **kw)


def test_preload_colormap_argument_errors():
    from unidepth_amd import preload_colormap
    with pytest.raises(ValueError, match="known: "):
        preload_colormap("no_such_map", "cuda:0")
    with pytest.raises(ValueError, match="must be a GPU"):
        preload_colormap("magma_r", "cpu")


def test_lazy_exports():
    import unidepth_amd
    from unidepth_amd import visualization
    for name in ("colorize", "colorize_batch", "demo_panel", "image_grid", "save_png", "preload_colormap"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(visualization, name)
    with pytest.raises(AttributeError):
        unidepth_amd.colourise


@pytest.mark.skipif(not os.path.isfile(mg.reference_path()), reason="reference tree not present (authoring machine only)")
def test_reference_rerun_reproduces_golden(golden):
    import matplotlib  # noqa: F401    where the reference tree is, matplotlib and PIL must be too: a missing one fails, never skips
    import PIL  # noqa: F401
    out = mg.reference_outputs(mg.reference_module())
    assert sorted(out) == sorted(golden)
    for name in out:
        np.testing.assert_array_equal(out[name], golden[name], err_msg=name)
