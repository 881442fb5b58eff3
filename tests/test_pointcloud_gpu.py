"""GPU tests of the point-cloud packing (csrc/pointcloud.hip through ud_pointcloud_pack and unidepth_amd/pointcloud.py) against the numpy
restatement of tools/make_golden_pointcloud.py (pinned to the reference's own arrays by tests/test_pointcloud_cpu.py).

The kernel tests call the C-ABI with every output inside a tests/layout_guard.py guard allocation: the guard bands and the rows at or
beyond the total must keep their bits.  Points mode is bit-exact.  Depth-mode x / y are three correctly rounded fp32 operations
((u - cx), * d, / fx) against the float64 restatement: 3 * layout_guard.term_store_f32, a bound derived from the arithmetic; z,
colours, indices, counts, offsets and the order are exact.  Shapes follow the kernel's constants: T = 1024 pixels per tile, S = 256
tile counts per scan sweep, 64 pixels per ballot word."""
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
assert_bound, guarded, term_store_f32 = lg.assert_bound, lg.guarded, lg.term_store_f32
_spec = importlib.util.spec_from_file_location("make_golden_pointcloud", os.path.join(ROOT, "tools", "make_golden_pointcloud.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

T, S = 1024, 256


def _guard(nbytes_rows, row_bytes, view_dtype):
    """`nbytes_rows` rows of `row_bytes` bytes inside a guard allocation, seen as a flat `view_dtype` tensor."""
    words = max(1, -(-nbytes_rows * row_bytes // 4))          # never an empty view: its address must be a real one at capacity 0 too
    g = guarded(words, 1, 1, torch.float32)
    return g, g.view.reshape(-1).view(view_dtype)


def _same_bits(a, b):
    """bitwise equality of two flat tensors (the untouched rows hold the guards' NaN pattern, which compares unequal as a float)"""
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Packed:
    pass


def _pack(points=None, depth=None, K=None, image=None, mask=None, confidence=None, min_confidence=None, depth_range=None, edge_rtol=None,
          flip_y=False, capacity=None, want_index=True):
    """ud_pointcloud_pack on guarded outputs, checked against restate(): returns the outputs (host) and the restatement."""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    ref = mg.restate(points, depth, K, image, mask, confidence, min_confidence, depth_range, edge_rtol, flip_y)
    total = int(ref["offsets"][-1])
    cap = total + 5 if capacity is None else capacity
    dev = {k: (None if v is None else torch.as_tensor(v).contiguous().cuda()) for k, v in
           dict(points=points, depth=depth, K=K, image=image, mask=mask, confidence=confidence).items()}
    lead = dev["points"] if dev["points"] is not None else dev["depth"]
    B, H, W = lead.shape[0], lead.shape[-2], lead.shape[-1]
    if dev["mask"] is not None and dev["mask"].dtype == torch.bool:
        dev["mask"] = dev["mask"].view(torch.uint8)
    img = dev.pop("image")
    f32_img = img is not None and img.dtype == torch.float32
    gx, xyz = _guard(cap, 12, torch.float32)
    gc, rgb = _guard(cap, 12 if f32_img else 3, torch.float32 if f32_img else torch.uint8)
    gi, index = _guard(cap, 4, torch.int32)
    gn, counts = _guard(B, 8, torch.int64)
    go, offsets = _guard(B + 1, 8, torch.int64)
    before = [t.clone() for t in (xyz, rgb, index)]
    nbytes = int(_lib.lib.ud_pointcloud_work_bytes(B, H, W))
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    flags = ((_lib.UD_PC_MINCONF if min_confidence is not None else 0) | (_lib.UD_PC_RANGE if depth_range is not None else 0) |
             (_lib.UD_PC_EDGE if edge_rtol is not None else 0) | (_lib.UD_PC_FLIP_Y if flip_y else 0))
    d = mk(_lib.UdPointCloud, xyz=xyz.data_ptr(), rgb=rgb.data_ptr() if img is not None else None, index=index.data_ptr() if want_index else None,
           counts=counts.data_ptr(), offsets=offsets.data_ptr(), work=work, work_bytes=nbytes, capacity=cap, B=B, H=H, W=W,
           nK=0 if dev["K"] is None else dev["K"].reshape(-1, 3, 3).shape[0], flags=flags,
           min_conf=0.0 if min_confidence is None else min_confidence, edge_rtol=0.0 if edge_rtol is None else edge_rtol,
           dmin=0.0 if depth_range is None else depth_range[0], dmax=0.0 if depth_range is None else depth_range[1],
           **{("image_f32" if f32_img else "image"): img}, **{k: v for k, v in dev.items() if v is not None})
    check(_lib.lib.ud_pointcloud_pack(d, cur_stream()), "ud_pointcloud_pack")
    torch.cuda.synchronize()
    for g in (gx, gc, gi, gn, go):
        g.check_guards()
    n = min(total, cap)
    r = Packed()
    r.ref, r.total, r.n, r.cap = ref, total, n, cap
    # rows at or beyond the total (and outputs that were not requested) keep their bits
    assert _same_bits(xyz[3 * n:], before[0][3 * n:])
    k = (3 * n) if img is not None else 0
    assert _same_bits(rgb[k:], before[1][k:])
    k = n if want_index else 0
    assert _same_bits(index[k:], before[2][k:])
    r.xyz = xyz[:3 * n].view(n, 3).cpu()
    r.rgb = rgb[:3 * n].view(n, 3).cpu() if img is not None else None
    r.index = index[:n].cpu() if want_index else None
    r.counts, r.offsets = counts.cpu(), offsets.cpu()
    # counts / offsets: the true totals whatever the capacity
    assert r.counts.tolist() == ref["counts"].tolist() and r.offsets.tolist() == ref["offsets"].tolist()
    if want_index:
        assert np.array_equal(r.index.numpy(), ref["index"][:n])
    if img is not None:
        assert r.rgb.numpy().dtype == ref["rgb"].dtype
        assert np.array_equal(r.rgb.numpy().view(np.uint8), np.ascontiguousarray(ref["rgb"][:n]).view(np.uint8))
    want = ref["xyz"][:n]
    if points is not None:                                       # bit-exact copies
        assert np.array_equal(r.xyz.numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    else:
        w64 = torch.from_numpy(np.ascontiguousarray(want))
        assert torch.equal(r.xyz[:, 2].double(), w64[:, 2])      # z = d
        assert_bound(r.xyz[:, :2], w64[:, :2], 3.0 * term_store_f32(w64[:, :2]), name="depth-mode x / y")
    return r


def _scene(B, H, W, seed, frac=0.6, f32_image=False):
    g = torch.Generator().manual_seed(seed)
    z = torch.exp(torch.randn(B, 1, H, W, generator=g) * 0.3 + 1.0)
    pts = torch.cat([torch.randn(B, 2, H, W, generator=g) * z, z], dim=1).float()
    image = torch.rand(B, 3, H, W, generator=g) if f32_image else torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    mask = torch.rand(B, H, W, generator=g) < frac
    conf = torch.rand(B, 1, H, W, generator=g)
    K = torch.tensor([[0.9 * W + 0.37, 0.0, W / 2 - 0.31], [0.0, 0.9 * W - 0.21, H / 2 + 0.17], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    K = K * (1.0 + 0.01 * torch.arange(B).view(B, 1, 1))
    K[:, 2, 2] = 1.0
    return dict(points=pts, depth=z[:, 0].contiguous(), image=image, mask=mask, confidence=conf, K=K.float())


SHAPES = [(1, 3, 5), (1, 1, 70), (1, 70, 1), (1, 8, 8), (1, 32, 32), (1, 25, 41), (1, 23, 89), (2, 37, 53), (1, 520, 520)]


@pytest.mark.parametrize("mode", ["points", "depth"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_shapes_by_kernel_constants(B, H, W, mode):
    """HW < 64, H = 1, W = 1, HW = 64, T, T + 1, 2T - 1, a width that makes waves straddle rows, and more than S tiles (two scan sweeps)"""
    assert (H * W) in (15, 70, 64, T, T + 1, 2 * T - 1, 37 * 53) or -(-H * W // T) > S
    s = _scene(B, H, W, seed=H * 1000 + W)
    if mode == "points":
        r = _pack(points=s["points"], image=s["image"], mask=s["mask"])
    else:
        r = _pack(depth=s["depth"], K=s["K"], image=s["image"], mask=s["mask"])
    assert 0 < r.total < B * H * W


@pytest.mark.parametrize("order", [("full", "empty", "sparse"), ("empty", "sparse", "full"), ("sparse", "full", "empty")])
def test_batch_with_empty_full_and_sparse_images(order):
    B, H, W = 3, 37, 53
    s = _scene(B, H, W, seed=11)
    g = torch.Generator().manual_seed(12)
    for b, kind in enumerate(order):
        s["mask"][b] = {"full": torch.ones(H, W, dtype=torch.bool), "empty": torch.zeros(H, W, dtype=torch.bool),
                        "sparse": torch.rand(H, W, generator=g) < 0.05}[kind]
    r = _pack(points=s["points"], image=s["image"], mask=s["mask"].view(torch.uint8) * 7)         # any nonzero byte is valid
    e, f = order.index("empty"), order.index("full")
    assert r.offsets[e] == r.offsets[e + 1] and r.counts[e] == 0 and r.counts[f] == H * W
    sp = order.index("sparse")
    assert 0 < r.counts[sp] < 0.1 * H * W
    _pack(depth=s["depth"], K=s["K"], mask=s["mask"])


def test_single_image_without_mask_is_every_pixel():
    s = _scene(1, 37, 53, seed=13)
    r = _pack(points=s["points"], image=s["image"])
    assert r.total == 37 * 53 and r.index.tolist() == list(range(37 * 53))


MIN_CONF, DMIN, DMAX, RTOL = 0.5, 2.5, 3.25, 0.0625


def _filter_scene(B=2, H=37, W=53, seed=21):
    """a smooth depth with flying pixels, NaN / inf in depth, points and confidence (corners, row ends, a tile border), and values exactly
    on min_conf, dmin, dmax and one ulp outside"""
    g = torch.Generator().manual_seed(seed)
    s = _scene(B, H, W, seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = (2.875 + 0.4 * torch.sin(yy / 9.0) * torch.cos(xx / 11.0)).repeat(B, 1, 1) * (1.0 + 0.004 * torch.randn(B, H, W, generator=g))
    fly = torch.rand(B, H, W, generator=g) < 0.04
    d = torch.where(fly, d * 1.5, d).float()
    flat = d.view(B, -1)
    one = np.float32(1.0)
    for b in range(B):
        p = torch.randperm(H * W, generator=g)
        flat[b, p[0:6]] = DMIN
        flat[b, p[6:12]] = DMAX
        flat[b, p[12:15]] = float(np.nextafter(np.float32(DMIN), -one))
        flat[b, p[15:18]] = float(np.nextafter(np.float32(DMAX), np.float32(10.0)))
        flat[b, p[18:22]] = float("nan")
        flat[b, p[22:26]] = float("inf")
        flat[b, p[26:28]] = float("-inf")
    d[0, 0, 0] = float("nan")
    d[0, H - 1, W - 1] = float("inf")
    d[1, 5, W - 1] = float("nan")                         # a row end: (6, 0) follows it in memory but is no neighbour
    d[1, T // W, T % W] = float("nan")                    # the first pixel of the second tile
    s["depth"] = d
    s["points"][:, 2] = d
    pf = s["points"].view(B, 3, -1)
    pf[0, 0, 100] = float("nan")                          # x / y not finite where z is fine
    pf[1, 1, 1500] = float("inf")
    cf = s["confidence"].view(B, -1)
    for b in range(B):
        p = torch.randperm(H * W, generator=g)
        cf[b, p[0:8]] = MIN_CONF
        cf[b, p[8:12]] = float(np.nextafter(np.float32(MIN_CONF), np.float32(0.0)))
        cf[b, p[12:16]] = float("nan")
    return s


FILTERS = {"minconf": dict(min_confidence=MIN_CONF), "range": dict(depth_range=(DMIN, DMAX)), "edge": dict(edge_rtol=RTOL), "none": {},
           "all": dict(min_confidence=MIN_CONF, depth_range=(DMIN, DMAX), edge_rtol=RTOL)}


@pytest.mark.parametrize("source", ["points", "points+depth", "depth"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_filters_alone_and_together(name, source):
    s = _filter_scene()
    f = FILTERS[name]
    kw = dict(mask=s["mask"], image=s["image"], confidence=s["confidence"] if "min_confidence" in f else None, **f)
    if source == "points":
        r = _pack(points=s["points"], **kw)
    elif source == "points+depth":                        # rows from points, the filters' d from the depth map (what from_prediction passes)
        s["points"][:, 2] += 100.0                        # z outside the range: a kernel that filtered on z would keep nothing
        r = _pack(points=s["points"], depth=s["depth"], **kw)
    else:
        r = _pack(depth=s["depth"], K=s["K"], **kw)
    nmask = int(s["mask"].sum())
    assert 0.05 * nmask < r.total < nmask                 # every filter (and the finite test alone) drops something and keeps something


def test_edge_filter_on_borders_row_ends_and_tile_borders():
    """steps on the image corners, at row ends (the next pixel in memory is not a neighbour), around the ballot-word border (pixels 63 / 64)
    and the tile border (pixels T - 1 / T); a step drops itself and its in-image 4-neighbours only"""
    H, W = 37, 53
    d = torch.ones(1, H, W)
    flat = d.view(-1)
    steps = [0, W - 1, (H - 1) * W, H * W - 1, 7 * W + W - 1, 12 * W, 63, 64 + 2 * W, T - 1, T + 3 * W, 30 * W + 20]
    flat[steps] = 2.0
    r = _pack(depth=d, K=torch.eye(3), edge_rtol=0.25)
    dropped = set(steps)
    for p in steps:
        y, x = divmod(p, W)
        dropped |= {q for q, ok in ((p - 1, x > 0), (p + 1, x < W - 1), (p - W, y > 0), (p + W, y < H - 1)) if ok}
    assert sorted(set(range(H * W)) - dropped) == r.index.tolist()
    assert 8 * W in r.index.tolist() and 12 * W - 1 in r.index.tolist()        # memory neighbours of row-end steps, kept


def test_edge_ramp_exactly_on_rtol():
    """d = 2^x: |d - dn| = min(d, dn) exactly, so edge_rtol = 1 keeps every pixel and the next float below 1 keeps none"""
    H, W = 3, 70
    d = (2.0 ** torch.arange(W, dtype=torch.float32)).repeat(1, H, 1)
    assert _pack(depth=d, K=torch.eye(3), edge_rtol=1.0).total == H * W
    assert _pack(depth=d, K=torch.eye(3), edge_rtol=float(np.nextafter(np.float32(1.0), np.float32(0.0)))).total == 0
    pts = torch.zeros(1, 3, H, W)
    pts[:, 2] = d
    assert _pack(points=pts, edge_rtol=1.0).total == H * W
    assert _pack(points=pts, edge_rtol=0.5).total == 0


@pytest.mark.parametrize("colour", ["u8", "f32", "none"])
@pytest.mark.parametrize("flip_y", [False, True])
@pytest.mark.parametrize("nK", [0, 1, 3])
def test_colour_flip_and_intrinsics_options(colour, flip_y, nK):
    B, H, W = 3, 25, 41
    s = _scene(B, H, W, seed=31, f32_image=colour == "f32")
    image = None if colour == "none" else s["image"]
    if nK == 0:
        r = _pack(points=s["points"], image=image, mask=s["mask"], flip_y=flip_y, want_index=colour != "none")
    else:
        r = _pack(depth=s["depth"], K=s["K"][:nK] if nK == 1 else s["K"], image=image, mask=s["mask"], flip_y=flip_y)
    assert r.total > 0
    if nK == 3:                                           # the per-image matrices differ: image 2's rows are not image 0's unprojection
        assert not torch.equal(s["K"][0], s["K"][2])


@pytest.mark.parametrize("mode", ["points", "depth"])
def test_capacity_below_the_total_and_zero(mode):
    B, H, W = 2, 37, 53
    s = _scene(B, H, W, seed=41)
    kw = dict(points=s["points"]) if mode == "points" else dict(depth=s["depth"], K=s["K"])
    full = _pack(image=s["image"], mask=s["mask"], **kw)
    cap = int(full.offsets[1]) + 17                       # cuts inside image 1, not on a word or tile border
    assert cap < full.total
    part = _pack(image=s["image"], mask=s["mask"], capacity=cap, **kw)
    assert part.n == cap and torch.equal(part.xyz, full.xyz[:cap]) and torch.equal(part.rgb, full.rgb[:cap])
    assert int(part.offsets[-1]) == full.total            # overflow is detectable
    none = _pack(image=s["image"], mask=s["mask"], capacity=0, **kw)
    assert none.n == 0 and int(none.offsets[-1]) == full.total


def _cloud_bits(pc):
    n = min(int(pc.offsets[-1]), pc.xyz.shape[0])
    parts = [pc.xyz[:n].view(torch.int32).cpu(), pc.counts.cpu(), pc.offsets.cpu()]
    parts += [t[:n].cpu() for t in (pc.rgb, pc.index) if t is not None]
    return parts


def test_two_runs_are_bitwise_equal():
    from unidepth_amd import pack_points
    s = {k: v.cuda() for k, v in _filter_scene(B=2, H=130, W=517, seed=51).items()}
    kw = dict(depth=s["depth"], image=s["image"], mask=s["mask"], confidence=s["confidence"], capacity=2 * 130 * 517, return_index=True, **FILTERS["all"])
    a = _cloud_bits(pack_points(s["points"], **kw))
    b = _cloud_bits(pack_points(s["points"], **kw))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[2][-1]) > 0
    kw.pop("depth")
    a = _cloud_bits(pack_points(depth=s["depth"], intrinsics=s["K"], **kw))
    b = _cloud_bits(pack_points(depth=s["depth"], intrinsics=s["K"], **kw))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _assert_cloud(pc, ref, n_rows=None):
    n = int(ref["offsets"][-1]) if n_rows is None else n_rows
    assert pc.counts.tolist() == ref["counts"].tolist() and pc.offsets.tolist() == ref["offsets"].tolist()
    assert np.array_equal(pc.xyz[:n].cpu().numpy().view(np.uint32), np.ascontiguousarray(ref["xyz"][:n]).view(np.uint32))
    if ref["rgb"] is not None:
        assert np.array_equal(pc.rgb[:n].cpu().numpy(), ref["rgb"][:n])
    if pc.index is not None:
        assert np.array_equal(pc.index[:n].cpu().numpy(), ref["index"][:n])


def test_pack_points_without_host_sync_when_capacity_is_given():
    from unidepth_amd import pack_points
    s = _filter_scene(seed=61)
    c = {k: v.cuda() for k, v in s.items()}
    work = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pc = pack_points(c["points"], depth=c["depth"], image=c["image"], mask=c["mask"], confidence=c["confidence"], capacity=5000,
                         return_index=True, workspace=work, **FILTERS["all"])
        pc2 = pack_points(depth=c["depth"].unsqueeze(1), intrinsics=c["K"], mask=c["mask"], capacity=100, flip_y=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = mg.restate(points=s["points"], depth=s["depth"], image=s["image"], mask=s["mask"], confidence=s["confidence"], **FILTERS["all"])
    assert pc.xyz.shape == (5000, 3) and pc.rgb.shape == (5000, 3) and pc.index.shape == (5000,) and 0 < int(ref["offsets"][-1]) < 5000
    _assert_cloud(pc, ref)
    assert pc2.xyz.shape == (100, 3) and int(pc2.offsets[-1]) > 100 and pc2.rgb is None and pc2.index is None


def test_pack_points_exact_allocation_split_and_input_forms():
    """capacity = None allocates exactly the total; split() gives per-image views; non-contiguous inputs, [B,1,H,W] / [B,H,W] maps and
    bool / uint8 masks give the same cloud"""
    from unidepth_amd import PointCloud, pack_points
    s = _scene(3, 25, 41, seed=71)
    s["mask"][1] = False
    ref = mg.restate(points=s["points"], image=s["image"], mask=s["mask"])
    c = {k: v.cuda() for k, v in s.items()}
    pc = pack_points(c["points"], image=c["image"], mask=c["mask"], return_index=True)
    assert isinstance(pc, PointCloud) and pc.xyz.shape == (int(ref["offsets"][-1]), 3) and pc.rgb.dtype == torch.uint8
    _assert_cloud(pc, ref)
    parts = pc.split()
    assert [p.xyz.shape[0] for p in parts] == ref["counts"].tolist() and parts[1].xyz.shape[0] == 0
    assert torch.equal(torch.cat([p.xyz for p in parts]), pc.xyz) and torch.equal(torch.cat([p.index for p in parts]), pc.index)
    assert parts[2].offsets.tolist() == [0, int(ref["counts"][2])]
    nhwc = c["points"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # the same values, channels-last strides
    assert not nhwc.is_contiguous()
    pc2 = pack_points(nhwc, image=c["image"], mask=c["mask"].view(torch.uint8).unsqueeze(1), return_index=True)
    assert all(torch.equal(x, y) for x, y in zip(_cloud_bits(pc), _cloud_bits(pc2)))
    empty = pack_points(c["points"], mask=torch.zeros_like(c["mask"]))
    assert empty.xyz.shape == (0, 3) and empty.offsets.tolist() == [0, 0, 0, 0]
    for kw in (dict(points=c["points"], mask=c["mask"].cpu()), dict(points=c["points"], confidence=c["confidence"][:, :, :-1], min_confidence=0.1)):
        with pytest.raises(ValueError):
            pack_points(**kw)


@pytest.mark.parametrize("name", list(mg.CASES))
def test_get_pointcloud_from_rgbd_matches_reference_golden(name):
    from unidepth_amd import get_pointcloud_from_rgbd
    image, depth, mask, K = mg.case_inputs(name)
    ref = np.load(mg.GOLDEN)[name]
    got = get_pointcloud_from_rgbd(image, depth[None], mask[..., None], K)          # squeezed, as the reference does
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(got[:, 2:], ref[:, 2:])                                    # z and colours exact, rows in the reference's order
    r64 = torch.from_numpy(ref[:, :2].copy())
    assert_bound(torch.from_numpy(got[:, :2].copy()), r64, 3.0 * term_store_f32(r64), name="x / y")
    with pytest.raises(NotImplementedError):
        get_pointcloud_from_rgbd(image, depth, mask, K, np.eye(4))


# ---- end to end: a real infer() output ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vits_prediction():
    """UniDepthV2 ViT-S (synthetic checkpoint) at 300x400, the smallest golden shape of oracle/cases.py: the model, two inputs, and the
    first one's infer() output on the host."""
    from oracle import cases, synth
    from unidepth_amd import UniDepthV2
    case = cases.CASES["vits_300x400_eucm"]
    cfg = synth.load_config(case["arch"])
    model = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, case["ckpt_seed"])).to("cuda").eval()
    rgbs = [torch.randint(0, 256, (1, 3, case["H"], case["W"]), dtype=torch.uint8, generator=torch.Generator().manual_seed(s)).cuda()
            for s in (case["img_seed"], case["img_seed"] + 100)]
    outs = [{k: v.clone() for k, v in model.infer(r).items()} for r in rgbs]
    torch.cuda.synchronize()
    return model, rgbs, outs


def _prediction_filters(out):
    thr = float(out["confidence"].float().median())
    lo, hi = (float(v) for v in torch.quantile(out["depth"].float().flatten(), torch.tensor([0.1, 0.9], device="cuda")))
    return dict(min_confidence=thr, depth_range=(lo, hi))


def test_from_prediction_on_infer_output(vits_prediction):
    from unidepth_amd import from_prediction
    model, rgbs, outs = vits_prediction
    out, rgb = outs[0], rgbs[0]
    f = _prediction_filters(out)
    pc = from_prediction(out, image=rgb, return_index=True, **f)
    host = {k: out[k].cpu() for k in ("points", "depth", "confidence")}
    ref = mg.restate(points=host["points"], depth=host["depth"], confidence=host["confidence"], image=rgb.cpu(), **f)
    n = int(ref["offsets"][-1])
    assert 0.1 * rgb.shape[-1] * rgb.shape[-2] < n < 0.6 * rgb.shape[-1] * rgb.shape[-2]
    _assert_cloud(pc, ref)
    gathered = host["points"][0].reshape(3, -1).t()[torch.from_numpy(ref["valid"][0].reshape(-1))]
    assert torch.equal(pc.xyz.cpu(), gathered)


def test_from_prediction_as_pipeline_post_hook(vits_prediction):
    """two requests in flight, each packing its own output on its own stream right behind infer(): the same bits as one at a time"""
    from unidepth_amd import from_prediction
    from unidepth_amd.pipeline import InferPipeline
    model, rgbs, outs = vits_prediction
    f = _prediction_filters(outs[0])
    cap = rgbs[0].shape[-1] * rgbs[0].shape[-2]
    alone = [_cloud_bits(from_prediction(o, image=r, capacity=cap, return_index=True, **f)) for o, r in zip(outs, rgbs)]
    torch.cuda.synchronize()
    pipe = InferPipeline(model, depth=2)
    clouds = []
    for r in rgbs:
        pipe.submit(r, post=lambda o, r=r: clouds.append(from_prediction(o, image=r, capacity=cap, return_index=True, **f)))
    pipe.sync()
    assert len(clouds) == 2
    for a, pc in zip(alone, clouds):
        assert int(a[2][-1]) > 0 and all(torch.equal(x, y) for x, y in zip(a, _cloud_bits(pc)))
