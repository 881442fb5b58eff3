"""GPU tests of the colourising (csrc/colorize.hip through ud_colorize and unidepth_amd/visualization.py) against the numpy restatement of
tools/make_golden_colorize.py (pinned to the reference's own bytes by tests/test_visualization_cpu.py).

The kernel tests call the C-ABI with the destination inside a tests/layout_guard.py guard allocation, at every byte offset 0..3 from a
4-byte boundary: the guard bands, the bytes around the destination and, in grid mode, the cells the call does not own must keep their
bits, and EVERY pixel must equal the restatement byte for byte -- no tolerance.  Shapes follow the kernel's constants (below)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(ROOT, "tests", "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)
_spec = importlib.util.spec_from_file_location("make_golden_colorize", os.path.join(ROOT, "tools", "make_golden_colorize.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

# csrc/colorize.hip
PX = 4                   # CZ_PX: pixels per thread
WAVE_PX = PX * 64        # CZ_PX * CZ_QUADS: pixels of a row per wave = width of a tile
ROWS = 4                 # CZ_ROWS: rows per tile; one workgroup renders ROWS x WAVE_PX pixels
CHUNK = 1024             # CZ_CHUNK: pixels per (min, max, has-NaN) partial
SWEEP = 256              # CZ_SWEEP: partials per reduction sweep
SLACK = 16               # bytes of the guarded view on either side of the destination


def _table(cmap):
    from unidepth_amd.colormaps import get_table
    return get_table(cmap)


def _u(B, H, W, seed, lo=-1.0, hi=12.0):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(B, H, W, generator=g)).float()


def _rgb(B, H, W, seed):
    return torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _render(B, H, W, rows, cols, panels, chw=False, off=0):
    """ud_colorize on a guarded destination `off` bytes past a 4-byte boundary, checked against restate().
    panels: None (cell left alone) | ("map", fp32 [B,H,W] host tensor or (device tensor, batch stride), vmin, vmax, cmap)
            | ("arel", g, p, vmin, vmax, cmap) | ("rgb", uint8 [B,3,H,W])."""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream
    n = B * rows * H * cols * W * 3
    words = -(-(n + 2 * SLACK + off) // 4)
    g = lg.guarded(words, 1, 1, torch.float32)
    view = g.view.reshape(-1).view(torch.uint8)
    before = view.clone()
    lo_b = SLACK + off
    d = _lib.UdColorize()
    d.dst = view.data_ptr() + lo_b
    d.B, d.H, d.W, d.rows, d.cols, d.flags = B, H, W, rows, cols, _lib.UD_CZ_CHW if chw else 0
    keep, want, auto = [], [], False
    for i, spec in enumerate(panels):
        if spec is None:
            want.append(None)
            continue
        p = d.panels[i]
        if spec[0] == "rgb":
            t = spec[1].cuda().contiguous()
            keep.append(t)
            p.kind, p.src, p.batch_stride = _lib.UD_CZ_RGB, t.data_ptr(), 3 * H * W
            want.append(spec[1].permute(0, 2, 3, 1).numpy())
            continue
        vmin, vmax, cmap = spec[-3:]
        if spec[0] == "map":
            if isinstance(spec[1], tuple):
                t, stride = spec[1]
            else:
                t, stride = spec[1].cuda().contiguous(), H * W
            vals = t.cpu().numpy()
            p.kind = _lib.UD_CZ_MAP
        else:
            t, stride = spec[1].cuda().contiguous(), H * W
            t2 = spec[2].cuda().contiguous()
            keep.append(t2)
            p.kind, p.src2, p.batch_stride2 = _lib.UD_CZ_AREL, t2.data_ptr(), H * W
            vals = np.stack([mg.arel(spec[1][b].numpy(), spec[2][b].numpy()) for b in range(B)])
        lut = torch.from_numpy(np.array(_table(cmap))).cuda()
        keep += [t, lut]
        p.src, p.batch_stride, p.lut = t.data_ptr(), stride, lut.data_ptr()
        p.flags = (_lib.UD_CZ_AUTO_LO if vmin is None else 0) | (_lib.UD_CZ_AUTO_HI if vmax is None else 0)
        auto = auto or p.flags != 0
        p.lo, p.hi = 0.0 if vmin is None else vmin, 0.0 if vmax is None else vmax
        p.den = float(vmax) - float(vmin) if p.flags == 0 else float("nan")
        want.append(np.stack([mg.restate(vals[b], _table(cmap), vmin, vmax) for b in range(B)]))
    if auto:
        nbytes = int(_lib.lib.ud_colorize_work_bytes(B, H, W))
        work = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")            # NaN bits: the scratch needs no initialisation
        d.work, d.work_bytes = work.data_ptr(), nbytes
    check(_lib.lib.ud_colorize(d, cur_stream()), "ud_colorize")
    torch.cuda.synchronize()
    g.check_guards()
    assert torch.equal(view[:lo_b], before[:lo_b]) and torch.equal(view[lo_b + n:], before[lo_b + n:]), "bytes around the destination rewritten"
    img = view[lo_b:lo_b + n].cpu().numpy().reshape((B, 3, rows * H, cols * W) if chw else (B, rows * H, cols * W, 3))
    was = before[lo_b:lo_b + n].cpu().numpy().reshape(img.shape)
    if chw:
        img, was = img.transpose(0, 2, 3, 1), was.transpose(0, 2, 3, 1)
    for i, w in enumerate(want):
        ys, xs = slice(i // cols * H, (i // cols + 1) * H), slice(i % cols * W, (i % cols + 1) * W)
        if w is None:
            assert np.array_equal(img[:, ys, xs], was[:, ys, xs]), f"cell {i} is not part of the call but was rewritten"
        else:
            bad = (img[:, ys, xs] != w).any(-1)
            assert not bad.any(), f"cell {i}: {int(bad.sum())} pixel(s) differ from the restatement, first at (b, y, x) = {tuple(np.argwhere(bad)[0])}"
    return img


SHAPES = [(1, 1), (3, 5), (7, 13), (24, 31),
          (2, PX - 1), (2, PX), (2, PX + 1), (2, WAVE_PX - 1), (2, WAVE_PX), (2, WAVE_PX + 1),
          (ROWS, WAVE_PX + 1), (ROWS + 1, WAVE_PX)]


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_by_kernel_constants(H, W, chw):
    """tiny and odd images (unaligned rows), W around the pixels-per-thread and per-wave multiples, one pixel column / row more than a
    workgroup renders; given limits and automatic ones; the destination at every offset from a 4-byte boundary"""
    v = _u(1, H, W, seed=H * 1000 + W)
    for off in range(4):
        _render(1, H, W, 1, 1, [("map", v, 0.01, 10.0, "magma_r")], chw=chw, off=off)
    _render(1, H, W, 1, 1, [("map", v, None, None, "coolwarm")], chw=chw, off=1)


def test_partials_one_more_than_a_sweep():
    H, W = 545, 481
    assert -(-H * W // CHUNK) == SWEEP + 1 and H * W < 300000
    v = _u(1, H, W, seed=5, lo=0.5, hi=9.0)
    v[0, H - 1, W - 1] = 11.0                       # the maximum lies in the last partial, the minimum in the first
    v[0, 0, 0] = 0.25
    img = _render(1, H, W, 1, 1, [("map", v, None, None, "magma_r")])
    assert img[0, 0, 0].tolist() == _table("magma_r")[0].tolist() and img[0, -1, -1].tolist() == _table("magma_r")[255].tolist()


@pytest.mark.parametrize("vmin,vmax", [(None, None), (0.5, None), (None, 30.0)])
def test_batch_of_three_auto_ranges(vmin, vmax):
    """the range is per image: three images of different spans in one call"""
    v = _u(3, 7, 13, seed=11, lo=0.5, hi=6.0) * torch.tensor([1.0, 2.0, 5.0]).view(3, 1, 1)
    img = _render(3, 7, 13, 1, 1, [("map", v, vmin, vmax, "magma_r")])
    whole = v.numpy()
    lo, hi = (float(whole.min()) if vmin is None else vmin), (float(whole.max()) if vmax is None else vmax)
    batch_wide = np.stack([mg.restate(whole[b], _table("magma_r"), lo, hi) for b in range(3)])
    assert (img != batch_wide).any()                # a batch-wide range would give other bytes


def test_strided_source_is_a_channel_of_points():
    """depth as channel 2 of a [B,3,H,W] points tensor, read in place through batch_stride"""
    B, H, W = 2, 7, 13
    pts = _u(B, 3 * H, W, seed=21).view(B, 3, H, W).cuda()
    depth = pts[:, 2]
    assert not depth.is_contiguous() and depth.data_ptr() == pts.data_ptr() + 2 * H * W * 4
    _render(B, H, W, 1, 1, [("map", (depth, 3 * H * W), None, 8.0, "viridis")], off=2)
    _render(B, H, W, 1, 1, [("map", (depth, 3 * H * W), 0.01, 10.0, "magma_r")], chw=True, off=3)
    from unidepth_amd import colorize_batch
    got = colorize_batch(depth, 0.01, 10.0).cpu().numpy()
    want = np.stack([mg.restate(depth[b].cpu().numpy(), _table("magma_r"), 0.01, 10.0) for b in range(B)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("chw", [False, True], ids=["hwc", "chw"])
def test_grids_at_odd_width(chw):
    """1 x 2 and 2 x 2 grids of all three panel kinds at W = 13: 3 W and 3 cols W are odd multiples, cell origins land on odd bytes;
    cells left out keep their bits"""
    B, H, W = 2, 7, 13
    g = _u(B, H, W, seed=31, lo=0.5, hi=8.0)
    p = (g * (0.8 + 0.4 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(32)))).float()
    g[:, ::3, ::2] = 0.0
    rgb = _rgb(B, H, W, seed=33)
    for off in range(4):
        _render(B, H, W, 2, 2, [("rgb", rgb), ("map", g, 0.01, 10.0, "magma_r"), ("map", p, 0.01, None, "magma_r"),
                                ("arel", g, p, 0.0, 0.2, "coolwarm")], chw=chw, off=off)
        _render(B, H, W, 1, 2, [("rgb", rgb), ("map", p, None, None, "turbo")], chw=chw, off=off)
        _render(1, 3, 5, 2, 2, [None, ("map", g[:1, :3, :5], 0.0, 5.0, "gray"), ("rgb", rgb[:1, :, :3, :5]), None], chw=chw, off=off)
    _render(1, 3, 5, 1, 4, [("arel", g[:1, :3, :5], p[:1, :3, :5], None, None, "Spectral_r"), None, ("rgb", rgb[:1, :, :3, :5]),
                            ("map", p[:1, :3, :5], None, 4.0, "inferno")], chw=chw, off=1)


@pytest.mark.parametrize("name", [n for n, c in mg.CASES.items() if c[0] != "f64"])
def test_golden_cases_equal_the_reference_bytes(name):
    """every fp32 case of the golden list (bin edges, vmax, out of range, the invalid threshold, NaN, +-inf, a constant image, the error
    map): the kernel's bytes are the reference's own"""
    kind, H, W, vmin, vmax, cmap = mg.CASES[name]
    if kind == "arel":
        g, p = (torch.from_numpy(a)[None] for a in mg.arel_inputs(name))
        img = _render(1, H, W, 1, 1, [("arel", g, p, vmin, vmax, cmap)], off=3)
    else:
        img = _render(1, H, W, 1, 1, [("map", torch.from_numpy(mg.case_inputs(name))[None], vmin, vmax, cmap)], off=3)
    assert np.array_equal(img[0], np.load(mg.GOLDEN)[name])


def _panel_restated(rgb, pred, gt=None):
    """demo_panel's default arguments restated per image -> uint8 [B, rows*H, cols*W, 3]."""
    out = []
    for b in range(rgb.shape[0]):
        cells = [rgb[b].transpose(1, 2, 0)]
        if gt is not None:
            cells.append(mg.restate(gt[b], _table("magma_r"), 0.01, 10.0))
        cells.append(mg.restate(pred[b], _table("magma_r"), 0.01, 10.0))
        if gt is not None:
            cells.append(mg.restate(mg.arel(gt[b], pred[b]), _table("coolwarm"), 0.0, 0.2))
        out.append(mg.restate_grid(cells, 2 if gt is not None else 1, 2))
    return np.stack(out)


def test_demo_panel_and_colorize_on_tensors():
    from unidepth_amd import colorize, colorize_batch, demo_panel
    B, H, W = 2, 24, 31
    gt = _u(B, H, W, seed=41, lo=0.2, hi=11.0)
    pred = (gt * (0.8 + 0.4 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(42)))).float()
    gt[:, ::4, ::5] = 0.0
    rgb = _rgb(B, H, W, seed=43)
    d_rgb, d_pred, d_gt = rgb.cuda(), pred.cuda()[:, None], gt.cuda()
    four = demo_panel(d_rgb, d_pred, d_gt)
    assert four.dtype == torch.uint8 and four.is_cuda and tuple(four.shape) == (B, 2 * H, 2 * W, 3)
    assert np.array_equal(four.cpu().numpy(), _panel_restated(rgb.numpy(), pred.numpy(), gt.numpy()))
    two = demo_panel(d_rgb, d_pred)
    assert tuple(two.shape) == (B, H, 2 * W, 3) and np.array_equal(two.cpu().numpy(), _panel_restated(rgb.numpy(), pred.numpy()))
    cf = demo_panel(d_rgb, d_pred, d_gt, channels_first=True)
    assert tuple(cf.shape) == (B, 3, 2 * H, 2 * W) and torch.equal(cf.permute(0, 2, 3, 1), four)
    one = demo_panel(d_rgb[0], d_pred[0, 0], d_gt[0])                                 # a single image without batch axes
    assert torch.equal(one, four[:1])
    # colorize keeps the reference's arguments: [H,W] -> [H,W,3], [B,H,W] and [B,1,H,W] -> [B,H,W,3]; None = per-image limits
    for vmin, vmax, cmap in ((0.01, 10.0, "magma_r"), (None, None, "coolwarm"), (1.0, None, "plasma")):
        want = np.stack([mg.restate(pred[b].numpy(), _table(cmap), vmin, vmax) for b in range(B)])
        assert np.array_equal(colorize(d_pred, vmin, vmax, cmap).cpu().numpy(), want)
        assert np.array_equal(colorize(d_pred[:, 0], vmin=vmin, vmax=vmax, cmap=cmap).cpu().numpy(), want)
        assert np.array_equal(colorize(d_pred[1, 0], vmin, vmax, cmap).cpu().numpy(), want[1])
        assert np.array_equal(colorize(pred[1].numpy(), vmin, vmax, cmap), want[1])                # the host path agrees
    out = torch.zeros(B, 3, H, W, dtype=torch.uint8, device="cuda")
    work = torch.empty(4 * B * 12 * -(-H * W // CHUNK), dtype=torch.uint8, device="cuda")
    ret = colorize_batch(d_pred, None, 9.0, "turbo", channels_first=True, out=out, workspace=work)
    assert ret is out
    want = np.stack([mg.restate(pred[b].numpy(), _table("turbo"), None, 9.0) for b in range(B)])
    assert np.array_equal(out.permute(0, 2, 3, 1).cpu().numpy(), want)
    with pytest.raises(ValueError):
        colorize_batch(d_pred, out=out)                                               # the HWC shape was asked for
    with pytest.raises(ValueError):
        colorize_batch(d_pred, workspace=work[:-1])
    with pytest.raises(ValueError):
        demo_panel(d_rgb, d_pred, gt)                                                 # a CPU tensor among GPU ones


@pytest.fixture(scope="module")
def vits_model():
    """UniDepthV2 ViT-S (synthetic checkpoint) at 300x400, the smallest golden shape of oracle/cases.py, and two inputs."""
    from oracle import cases, synth
    from unidepth_amd import UniDepthV2
    case = cases.CASES["vits_300x400_eucm"]
    cfg = synth.load_config(case["arch"])
    model = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, case["ckpt_seed"])).to("cuda").eval()
    rgbs = [torch.randint(0, 256, (1, 3, case["H"], case["W"]), dtype=torch.uint8, generator=torch.Generator().manual_seed(s)).cuda()
            for s in (case["img_seed"], case["img_seed"] + 100)]
    return model, rgbs


def test_demo_panel_as_pipeline_post_hook(vits_model):
    """two requests in flight, each rendering its own panel on its own stream right behind infer(): the same bytes as the panel made
    from the finished output, which equal the restatement"""
    from unidepth_amd import demo_panel
    from unidepth_amd.pipeline import InferPipeline
    model, rgbs = vits_model
    pipe = InferPipeline(model, depth=2)
    panels, outs = [], []
    for r in rgbs:
        outs.append(pipe.submit(r, post=lambda o, r=r: panels.append(demo_panel(r, o["depth"], depth_range=(None, None)))))
    for o in outs:
        pipe.wait(o)
    assert len(panels) == 2
    for r, o, p in zip(rgbs, outs, panels):
        after = demo_panel(r, o["depth"], depth_range=(None, None))
        torch.cuda.synchronize()
        assert torch.equal(p, after)
        d = o["depth"].reshape(1, *o["depth"].shape[-2:]).cpu().numpy()
        want = mg.restate_grid([r[0].permute(1, 2, 0).cpu().numpy(), mg.restate(d[0], _table("magma_r"))], 1, 2)
        assert np.array_equal(p[0].cpu().numpy(), want) and len(np.unique(want[:, want.shape[1] // 2:].reshape(-1, 3), axis=0)) > 50


def test_preload_colormap_uploads_the_table_once():
    """preload_colormap puts the table on the device; the calls that follow use that very tensor (no second upload, so no wait)"""
    from unidepth_amd import colorize_batch, preload_colormap, visualization
    dev = torch.device("cuda", torch.cuda.current_device())
    visualization._LUTS.pop(("Spectral_r", str(dev)), None)
    for device in (None, "cuda", dev):
        preload_colormap("Spectral_r", device)
    assert [k for k in visualization._LUTS if k[0] == "Spectral_r"] == [("Spectral_r", str(dev))]
    t = visualization._LUTS[("Spectral_r", str(dev))]
    assert t.device == dev and np.array_equal(t.cpu().numpy(), _table("Spectral_r"))
    v = _u(1, 7, 13, 77)
    got = colorize_batch(v.cuda(), 0.0, 10.0, "Spectral_r")
    assert visualization._LUTS[("Spectral_r", str(dev))] is t
    assert np.array_equal(got[0].cpu().numpy(), mg.restate(v[0].numpy(), _table("Spectral_r"), 0.0, 10.0))
