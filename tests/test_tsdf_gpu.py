"""GPU parity of tsdf_integrate (unidepth_amd/tsdf.py -> ud_tsdf_integrate, csrc/tsdf.hip) against tsdf_integrate_composition --
project_camera, remap(mode="nearest") and torch element-wise arithmetic in a loop over the views -- bit for bit in tsdf, weight, colour and
count at every voxel, compared as integers: both sides run the same functions of camera_models.h and remap_taps.h under
-ffp-contract=off.  tsdf_points (ud_tsdf_points) is compared with the numpy restatement of ud_tsdf_slot in tests/tsdf_common.py.  The
scenes are those of tests/tsdf_common.py, whose shares tests/test_tsdf_cpu.py asserts on the host program; the raw C-ABI calls write into
guarded allocations (tests/layout_guard.py), fp32 outputs off 16-byte boundaries and uint8 outputs at odd byte offsets."""
import functools

import numpy as np
import pytest
import torch

import layout_guard as lg
import tsdf_common as tc

pytestmark = pytest.mark.gpu
_SENTINEL_BYTES = (0xAD, 0xDB, 0xBA, 0x7F)                     # lg.SENTINEL[torch.float32], little endian
SETS = {**{tc.NAMES[m]: m for m in tc.MODELS}, "mixed": tc.mixed_models()}
OPTION_SETS = ({}, dict(src_masks=True), dict(src_weights=True), dict(images=True), dict(max_weight=tc.MAX_WEIGHT),
               dict(src_masks=True, src_weights=True, images=True, max_weight=tc.MAX_WEIGHT))
ALL = OPTION_SETS[-1]


class _Out:
    """`n` elements of `dtype`, `offset` elements into a sentinel-filled allocation: the guard rows above and below are checked by
    layout_guard, the bytes of the view's own words before and after the elements here"""

    def __init__(self, n, dtype, offset=0):
        esz = torch.empty(0, dtype=dtype).element_size()
        self.words = max(1, -(-(n + offset) * esz // 4))
        self.g = lg.guarded(self.words, 1, 1, torch.float32)
        self.bytes = self.g.view.reshape(-1).view(torch.uint8)
        self.lo, self.hi = offset * esz, (offset + n) * esz
        self.t = self.bytes[self.lo:self.hi].view(dtype)

    def check(self, name, written=True, upto=None):
        """guards intact; with `upto` (elements) only the first upto elements may have been written"""
        self.g.check_guards(name)
        want = torch.tensor(_SENTINEL_BYTES, dtype=torch.uint8, device="cuda").repeat(self.words)
        keep = torch.ones_like(want, dtype=torch.bool)
        if written:
            hi = self.hi if upto is None else self.lo + upto * self.t.element_size()
            keep[self.lo:hi] = False
        assert torch.equal(self.bytes[keep], want[keep]), f"{name}: bytes beside the output were rewritten" if written else f"{name}: an absent output was written"


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _to_device(s):
    d = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()}
    d["cams"] = [tc.prepared(s["params"][v], s["models"][v]) for v in range(s["V"])]
    return d


@functools.lru_cache(maxsize=None)
def _device_scene(**kw):
    """a scene of tsdf_common on the GPU (shared, never written): tensors, and the cameras as PreparedCamera"""
    return _to_device(tc.scene(**kw))


def _call(f, d, volume=None, views=slice(None), src_masks=False, src_weights=False, images=False, max_weight=None, return_count=True):
    T = d["T"][views] if d["T"].ndim == 3 else d["T"][:, views]
    kw = dict(trunc=d["trunc"], max_weight=max_weight, return_count=return_count)
    if volume is None:
        kw.update(grid_shape=d["grid"], origin=d["origin"], voxel_size=d["voxel"])
    for name, on in (("src_masks", src_masks), ("src_weights", src_weights), ("images", images)):
        if on:
            kw[name] = d[name][:, views]
    return f(volume, d["depths"][:, views], d["cams"][views], T, **kw)


def _outputs(res):
    vol, count = res
    return vol.tsdf, vol.weight, vol.color, count


def _clone(vol):
    from unidepth_amd import tsdf
    return tsdf.TsdfVolume(vol.tsdf.clone(), vol.weight.clone(), None if vol.color is None else vol.color.clone(), vol.origin, vol.voxel_size)


def _both(d, what, volume=None, **kw):
    """the fused call and the composition on the same arguments (each on its own copy of a given volume), every output compared bit for
    bit -> the fused call's (volume, count)"""
    from unidepth_amd import tsdf
    got = _call(tsdf.tsdf_integrate, d, None if volume is None else _clone(volume), **kw)
    want = _call(tsdf.tsdf_integrate_composition, d, None if volume is None else _clone(volume), **kw)
    Nz, Ny, Nx = d["grid"]
    assert got[0].tsdf.shape == (d["B"], Nz, Ny, Nx) and got[1].dtype == torch.uint8 and (got[0].color is not None) == bool(kw.get("images"))
    tc.host_program.assert_same(_outputs(got), _outputs(want), tc.OUTPUTS, what)
    return got


def _check_points(vol, what, min_weight=1.0):
    """tsdf_points on the volume, u8 and fp32 colours, against the numpy restatement, bit for bit -> the number of points"""
    from unidepth_amd import tsdf
    live, xyz, rgb = tc.slots(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.color is None else vol.color.cpu().numpy(),
                              vol.origin.cpu().numpy(), vol.voxel_size, min_weight)
    wx, wr, wc, wo = tc.packed(live, xyz, rgb)
    for dtype in (torch.uint8, torch.float32):
        pc = tsdf.tsdf_points(vol, min_weight=min_weight, rgb_dtype=dtype)
        assert pc.index is None and np.array_equal(pc.counts.cpu().numpy(), wc) and np.array_equal(pc.offsets.cpu().numpy(), wo), what
        assert pc.xyz.shape == (int(wo[-1]), 3) and tc.host_program.same_bits(pc.xyz.cpu().numpy(), wx), what
        if rgb is None:
            assert pc.rgb is None
        else:
            assert pc.rgb.dtype == dtype and tc.host_program.same_bits(pc.rgb.cpu().numpy(), tc.to_u8(wr) if dtype == torch.uint8 else wr), what
    return int(wo[-1])


# ---- fused against composition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SETS))
def test_fused_equals_composition(name):
    """each of the six models as the view model, and one batch mixing all six: B = 2, V = 3 on the base scene, shared and per-image
    transforms and origins, each optional input on and off, a fresh and a continued volume: tsdf, weight, colour and count bit-equal"""
    from unidepth_amd import tsdf
    for per in (False, True):
        d = _device_scene(models=SETS[name], per_image=per, per_origin=per, **tc.BASE)
        plain = None
        for opts in OPTION_SETS:
            vol, count = _both(d, f"{name} per={per} {sorted(opts)}", **opts)
            assert bool(count.any()) and not bool((count == d["V"]).all())
            if plain is None:
                plain = vol
            elif set(opts) != {"images"}:                                       # the optional inputs are read
                assert not torch.equal(vol.weight, plain.weight) or not torch.equal(tc.bits(vol.tsdf), tc.bits(plain.tsdf))
        for opts in (ALL, {}):
            first, _ = _call(tsdf.tsdf_integrate, d, views=slice(0, 1), **opts)
            _both(d, f"{name} per={per} continued {sorted(opts)}", volume=first, views=slice(1, 3), **opts)
        assert _check_points(vol, name, min_weight=0.75) > 0


@pytest.mark.parametrize("max_weight", (None, tc.MAX_WEIGHT))
def test_split_property(max_weight):
    """V views in one call equal the first k and then the rest in two calls, bit for bit, with and without max_weight"""
    from unidepth_amd import tsdf
    d = _device_scene(models=tc.mixed_models(), per_image=True, **tc.BASE)
    opts = dict(src_weights=True, images=True, src_masks=True, max_weight=max_weight)
    whole, count = _call(tsdf.tsdf_integrate, d, **opts)
    for k in (1, 2):
        vol, c0 = _call(tsdf.tsdf_integrate, d, views=slice(0, k), **opts)
        same, c1 = _call(tsdf.tsdf_integrate, d, vol, views=slice(k, 3), **opts)
        assert same is vol
        tc.host_program.assert_same((vol.tsdf, vol.weight, vol.color, c0 + c1), (whole.tsdf, whole.weight, whole.color, count), tc.OUTPUTS, f"k={k}")
    assert bool((count == 3).any()) and bool((whole.weight <= tc.MAX_WEIGHT).all()) == (max_weight is not None)


@pytest.mark.parametrize("name", list(tc.EDGES))
def test_edges(name):
    """Nx in {1, 63, 64, 65, 255, 257} with Ny, Nz in {1, 2}; a 1x1x1 grid; 1x1 and 2x3 views; V = 1; B = 32 with V = 8 on a 3x3x3 grid"""
    d = _device_scene(**tc.EDGES[name])
    vol, count = _both(d, name, **ALL)
    assert bool(count.any())
    _check_points(vol, name, min_weight=0.5)
    vol, _ = _both(d, name + " plain")
    _check_points(vol, name + " plain", min_weight=0.5)


def test_python_surface():
    """camera objects and prepared cameras, 4x4 and 3x4 transforms, other float dtypes converted, bool and uint8 masks, the origin as
    numbers, without return_count: the same bits"""
    import remap_common
    from unidepth_amd import cameras, tsdf
    gp = remap_common.gp
    s = tc.scene(tc.mixed_models(), per_image=True, **tc.BASE)
    d = _device_scene(models=tc.mixed_models(), per_image=True, **tc.BASE)
    base, count = _both(d, "mixed", **ALL)
    cams = [cameras.BatchCamera([gp.make_camera(cameras, m, r) for m, r in zip(s["models"][v], s["params"][v])]) for v in range(s["V"])]
    T44 = torch.eye(4, device="cuda").repeat(s["B"], s["V"], 1, 1)
    T44[:, :, :3] = d["T"]
    vol = tsdf.tsdf_integrate(None, d["depths"].double(), tuple(cams), T44, grid_shape=list(s["grid"]), origin=tuple(float(x) for x in s["origin"][0]),
                              voxel_size=s["voxel"], trunc=s["trunc"], src_masks=d["src_masks"].bool(), src_weights=d["src_weights"].double(),
                              images=d["images"], max_weight=tc.MAX_WEIGHT)
    assert isinstance(vol, tsdf.TsdfVolume) and vol.voxel_size == s["voxel"] and vol.origin.shape == (1, 3)
    tc.host_program.assert_same((vol.tsdf, vol.weight, vol.color), (base.tsdf, base.weight, base.color), tc.OUTPUTS[:3], "objects")
    # a given volume must be contiguous fp32 on the GPU and fit the call
    for bad in (tsdf.TsdfVolume(vol.tsdf[:, :, :, ::2], vol.weight, vol.color, vol.origin, vol.voxel_size),
                tsdf.TsdfVolume(vol.tsdf.double(), vol.weight, vol.color, vol.origin, vol.voxel_size),
                tsdf.TsdfVolume(vol.tsdf, vol.weight[:1], vol.color, vol.origin, vol.voxel_size),
                tsdf.TsdfVolume(vol.tsdf, vol.weight, None, vol.origin, vol.voxel_size),
                tsdf.TsdfVolume(vol.tsdf, vol.weight, vol.color, vol.origin.cpu(), vol.voxel_size),
                tsdf.TsdfVolume(vol.tsdf[:1], vol.weight[:1], vol.color[:1], vol.origin, vol.voxel_size)):
        with pytest.raises(ValueError, match="tsdf_integrate: "):
            _call(tsdf.tsdf_integrate, d, bad, **ALL)
    for kw in (dict(min_weight="x"), dict(min_weight=float("nan")), dict(capacity=-1), dict(capacity=1.5), dict(capacity=True),
               dict(rgb_dtype=torch.float16), dict(workspace=torch.empty(8, dtype=torch.uint8, device="cuda")),
               dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device="cuda")), dict(workspace=bytearray(1 << 20)),
               dict(workspace=torch.empty(1 << 20, dtype=torch.uint8, device="cuda")[1:])):
        with pytest.raises(ValueError, match="tsdf_points: "):
            tsdf.tsdf_points(vol, **kw)


# ---- known answer and special values --------------------------------------------------------------------------------------------------

def test_known_answer():
    """one Pinhole view, identity transform, constant depth 2, centres on multiples of 0.125: tsdf = min(1, (2 - z) / 0.5) exactly where
    2 - z >= -0.5 and untouched behind that; tsdf_points gives only points with z == 2.0 exactly"""
    from unidepth_amd import tsdf
    d = _to_device(tc.known_answer_scene())
    vol, count = _both(d, "known answer")
    pc = tsdf.tsdf_points(vol)
    n = int(np.prod(d["grid"]))
    live = np.zeros((1, 3 * n), bool)
    live[0, :pc.xyz.shape[0]] = True
    xyz = np.zeros((1, 3 * n, 3), np.float32)
    xyz[0, :pc.xyz.shape[0]] = pc.xyz.cpu().numpy()
    tc.check_known_answer(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), count.cpu().numpy(), live, xyz)
    _check_points(vol, "known answer")


@pytest.mark.parametrize("weights", (False, True))
def test_special_values(weights):
    """NaN, +-inf, 0, -0.0 and negatives in the depths; NaN, 0, inf and negatives in the weights; voxels behind every view; a singular
    Pinhole row: fused equals composition bit for bit and no voxel is updated that its inputs cannot support"""
    s = tc.special_scene()
    d = _to_device(s)
    for masks in (False, True):
        vol, count = _both(d, f"special masks={masks}", src_masks=masks, src_weights=weights, images=True)
        r = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), count=count.cpu().numpy())
        tc.check_special(r, s, weights)
        _check_points(vol, "special", min_weight=0.5)


# ---- tsdf_points against the numpy restatement ----------------------------------------------------------------------------------------

def _planted(B, nx, seed, empty=None):
    """a volume of B rows of nx voxels with random distances (a few NaN), weights in {0, 1, 2} and colours; volume `empty` has no weight"""
    from unidepth_amd import tsdf
    return tsdf.TsdfVolume(*(_dev(x) for x in tc.planted(B, (1, 1, nx), seed, empty)), tc.f32(0.05))


@pytest.mark.parametrize("nx", (341, 342, 683))
def test_points_around_the_tile(nx):
    """1023, 1026 and 2049 slots, around the tile of 1024: bit for bit in xyz, rgb (u8 and fp32), counts and offsets; B = 3 with one empty
    volume; a capacity below the total keeps the counts true and the rows past it untouched; min_weight above every weight: empty"""
    from unidepth_amd import tsdf
    vol = _planted(3, nx, nx, empty=1)
    total = _check_points(vol, f"nx={nx}")
    pc = tsdf.tsdf_points(vol)
    assert total > 20 and int(pc.counts[1]) == 0 and int(pc.counts[0]) > 0 and int(pc.counts[2]) > 0
    cap = total - 7
    part = tsdf.tsdf_points(vol, capacity=cap, workspace=torch.full((1 << 16,), 0xFF, dtype=torch.uint8, device="cuda"))
    assert torch.equal(part.counts, pc.counts) and torch.equal(part.offsets, pc.offsets) and part.xyz.shape == (cap, 3)
    assert torch.equal(tc.bits(part.xyz), tc.bits(pc.xyz[:cap])) and torch.equal(part.rgb, pc.rgb[:cap])
    none = tsdf.tsdf_points(vol, min_weight=2.5)
    assert none.xyz.shape == (0, 3) and none.rgb.shape == (0, 3) and not bool(none.counts.any()) and not bool(none.offsets.any())
    big = tsdf.tsdf_points(vol, capacity=total + 5)                               # rows past the total stay unwritten; the written ones agree
    assert torch.equal(tc.bits(big.xyz[:total]), tc.bits(pc.xyz)) and torch.equal(big.offsets, pc.offsets)


def test_points_over_more_than_256_tiles():
    """257 tiles per volume: the scan of a volume's tile counts takes a second chunk with the carry of the first.  B = 2 different
    volumes with colours, live slots in the tiles 0, 255 and 256 (asserted on the restatement before the GPU is asked); bit for bit as
    above, and a capacity below the total"""
    from unidepth_amd import tsdf
    arrays, voxel = tc.many_tiles_volumes()
    vol = tsdf.TsdfVolume(*(_dev(x) for x in arrays), voxel)
    total = _check_points(vol, "257 tiles")
    pc = tsdf.tsdf_points(vol)
    cap = total // 2
    part = tsdf.tsdf_points(vol, capacity=cap)
    assert cap > 1024 and torch.equal(part.counts, pc.counts) and torch.equal(part.offsets, pc.offsets) and part.xyz.shape == (cap, 3)
    assert torch.equal(tc.bits(part.xyz), tc.bits(pc.xyz[:cap])) and torch.equal(part.rgb, pc.rgb[:cap])


# ---- guarded C-ABI ------------------------------------------------------------------------------------------------------------------

def _raw_integrate(d, state=None, count=True, **opts):
    """ud_tsdf_integrate through the C-ABI, every output inside a guarded allocation (absent ones too: they must stay untouched), twice
    from the same state -> (tsdf, weight, color or None, count or None)"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    B, V = d["B"], d["V"]
    Nz, Ny, Nx = d["grid"]
    n = B * Nz * Ny * Nx
    images = bool(opts.get("images"))
    bufs = dict(tsdf=_Out(n, torch.float32, 1), weight=_Out(n, torch.float32, 3), color=_Out(3 * n, torch.float32, 1), count=_Out(n, torch.uint8, 3))
    has = dict(tsdf=True, weight=True, color=images, count=count)
    T = d["T"].reshape(-1, V, 3, 4).contiguous()
    mw = opts.get("max_weight")
    src, params = d["depths"].contiguous(), torch.stack([c.params for c in d["cams"]])      # held until the calls are over
    desc = mk(_lib.UdTsdfIntegrate, src_depth=src, src_mask=d["src_masks"] if opts.get("src_masks") else None,
              src_weight=d["src_weights"] if opts.get("src_weights") else None, image=d["images"] if images else None,
              params=params, T=T, origin=d["origin"], B=B, V=V, Nx=Nx, Ny=Ny, Nz=Nz, Hs=d["Hs"], Ws=d["Ws"],
              nT=T.shape[0], n_origin=d["origin"].shape[0], fresh=int(state is None), has_max_weight=int(mw is not None),
              voxel_size_bits=tc.f32_bits(d["voxel"]), trunc_bits=tc.f32_bits(d["trunc"]), max_weight_bits=tc.f32_bits(mw or 0.0),
              **{k: (b.t.data_ptr() if has[k] else None) for k, b in bufs.items()})
    for v in range(V):
        for b in range(B):
            desc.model[v * B + b] = d["cams"][v].models[b]
    runs = []
    for _ in range(2):
        if state is not None:
            bufs["tsdf"].t.copy_(state.tsdf.reshape(-1))
            bufs["weight"].t.copy_(state.weight.reshape(-1))
            if images:
                bufs["color"].t.copy_(state.color.reshape(-1))
        check(_lib.lib.ud_tsdf_integrate(desc, cur_stream()), "ud_tsdf_integrate")
        torch.cuda.synchronize()
        runs.append({k: b.t.clone() for k, b in bufs.items() if has[k]})
    for k, b in bufs.items():
        b.check(k, has[k])
    for k in runs[0]:
        assert torch.equal(tc.bits(runs[0][k]), tc.bits(runs[1][k])), f"two calls gave different bits in {k}"
    r = runs[0]
    shape = (B, Nz, Ny, Nx)
    return (r["tsdf"].view(shape), r["weight"].view(shape), r["color"].view(B, 3, Nz, Ny, Nx) if images else None, r["count"].view(shape) if count else None)


def test_guarded_integrate():
    """the entry point itself on guarded allocations off 16-byte boundaries: absent optional outputs stay untouched, guard bytes stay
    intact, a fresh call reads nothing of its outputs' sentinels, two calls give the same bits, and the bits are the wrapper's"""
    from unidepth_amd import tsdf
    for kw in (dict(models=tc.mixed_models(), per_image=True, per_origin=True, **tc.BASE), tc.EDGES["nx257_2_1"], tc.EDGES["src1x1"]):
        d = _device_scene(**kw)
        for opts in (ALL, {}, dict(src_weights=True)):
            want = _call(tsdf.tsdf_integrate, d, **opts)
            tc.host_program.assert_same(_raw_integrate(d, **opts), _outputs(want), tc.OUTPUTS, f"raw {sorted(opts)}")
            part = _raw_integrate(d, count=False, **opts)
            tc.host_program.assert_same(part[:3], _outputs(want)[:3], tc.OUTPUTS[:3], "raw without count")
            first, _ = _call(tsdf.tsdf_integrate, d, views=slice(0, 1), **opts)
            e = dict(d, V=d["V"] - 1, depths=d["depths"][:, 1:].contiguous(), src_masks=d["src_masks"][:, 1:].contiguous(), src_weights=d["src_weights"][:, 1:].contiguous(),
                     images=d["images"][:, 1:].contiguous(), cams=d["cams"][1:], T=(d["T"][1:] if d["T"].ndim == 3 else d["T"][:, 1:]))
            if e["V"]:
                tc.host_program.assert_same(_raw_integrate(e, state=first, **opts)[:3], _outputs(want)[:3], tc.OUTPUTS[:3], "raw continued")


def test_guarded_points():
    """ud_tsdf_points on guarded allocations: xyz and fp32 rgb off 16-byte boundaries, u8 rgb at an odd offset, a dirty workspace, a
    capacity below the total (rows past it keep their guard bits), absent outputs untouched"""
    from unidepth_amd import _lib, tsdf
    from unidepth_amd.ops import check, cur_stream, mk
    vol = _planted(3, 683, 1, empty=2)
    want = tsdf.tsdf_points(vol, rgb_dtype=torch.float32)
    want8 = tsdf.tsdf_points(vol)
    total = want.xyz.shape[0]
    need = int(_lib.lib.ud_tsdf_points_work_bytes(3, 683, 1, 1))
    for f32, with_rgb, cap in ((0, True, total), (1, True, total - 5), (0, False, total), (0, True, 0)):
        bufs = dict(xyz=_Out(3 * max(cap, 1), torch.float32, 1), rgb=_Out(3 * max(cap, 1), torch.float32 if f32 else torch.uint8, 3),
                    counts=_Out(3, torch.int64, 1), offsets=_Out(4, torch.int64, 1))
        work = torch.full((need + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        desc = mk(_lib.UdTsdfPoints, tsdf=vol.tsdf, weight=vol.weight, color=vol.color, origin=vol.origin, xyz=bufs["xyz"].t.data_ptr() if cap else None,
                  rgb=bufs["rgb"].t.data_ptr() if (with_rgb and cap) else None, counts=bufs["counts"].t.data_ptr(), offsets=bufs["offsets"].t.data_ptr(),
                  work=work, work_bytes=need, capacity=cap, B=3, Nx=683, Ny=1, Nz=1, n_origin=3, rgb_f32=f32,
                  voxel_size_bits=tc.f32_bits(vol.voxel_size), min_weight_bits=tc.f32_bits(1.0))
        check(_lib.lib.ud_tsdf_points(desc, cur_stream()), "ud_tsdf_points")
        torch.cuda.synchronize()
        assert bool((work[need:] == 0xFF).all())
        assert torch.equal(bufs["counts"].t, want.counts) and torch.equal(bufs["offsets"].t, want.offsets)
        bufs["counts"].check("counts")
        bufs["offsets"].check("offsets")
        bufs["xyz"].check("xyz", written=cap > 0, upto=3 * cap)
        bufs["rgb"].check("rgb", written=with_rgb and cap > 0, upto=3 * cap)
        if cap:
            assert torch.equal(tc.bits(bufs["xyz"].t[:3 * cap].view(cap, 3)), tc.bits(want.xyz[:cap]))
            if with_rgb:
                ref = want.rgb if f32 else want8.rgb
                assert torch.equal(tc.bits(bufs["rgb"].t[:3 * cap].view(cap, 3)), tc.bits(ref[:cap]))


# ---- graph replay ------------------------------------------------------------------------------------------------------------------

def test_graph_replay_after_inputs_were_rewritten():
    """both calls captured once with PreparedCameras; replayed after depths, weights, transforms and camera rows were rewritten in place:
    each replay equals the eager results and the composition"""
    from unidepth_amd import gtpoints, tsdf
    kw = dict(models=tc.mixed_models(), per_image=True, **tc.BASE)
    d, e = _device_scene(**kw), _device_scene(seed=3, **kw)
    depths, weights, T = d["depths"].clone(), d["src_weights"].clone(), d["T"].clone()
    cams = [gtpoints.PreparedCamera(c.params.clone(), c.models) for c in d["cams"]]
    opts = dict(grid_shape=d["grid"], origin=d["origin"], voxel_size=d["voxel"], trunc=d["trunc"], src_masks=d["src_masks"], src_weights=weights,
                images=d["images"], max_weight=tc.MAX_WEIGHT, return_count=True)
    n_slots = 3 * int(np.prod(d["grid"])) * d["B"]

    def fn():
        vol, count = tsdf.tsdf_integrate(None, depths, cams, T, **opts)
        return vol, count, tsdf.tsdf_points(vol, min_weight=0.75, capacity=n_slots)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        svol, scount, spc = fn()
    for k in range(3):
        depths.copy_(e["depths"] if k % 2 == 0 else d["depths"])
        weights[:, 1].copy_(e["src_weights"][:, 1] if k % 2 == 0 else d["src_weights"][:, 1])
        T[1, 2].copy_(e["T"][1, 2] if k % 2 == 0 else d["T"][1, 2])
        cams[0].params[1, :2].mul_(1.02 if k % 2 == 0 else 0.97)
        cams[2].params[0, 2:4].add_(0.25 if k % 2 == 0 else -0.125)
        graph.replay()
        torch.cuda.synchronize()
        vol, count, pc = fn()
        total = int(pc.offsets[-1])
        tc.host_program.assert_same((svol.tsdf, svol.weight, svol.color, scount), (vol.tsdf, vol.weight, vol.color, count), tc.OUTPUTS, f"replay {k}")
        tc.host_program.assert_same((spc.xyz[:total], spc.rgb[:total], spc.counts, spc.offsets), (pc.xyz[:total], pc.rgb[:total], pc.counts, pc.offsets),
                                    ("xyz", "rgb", "counts", "offsets"), f"replay {k} points")
        want = tsdf.tsdf_integrate_composition(None, depths, cams, T, **opts)
        tc.host_program.assert_same((svol.tsdf, svol.weight, svol.color, scount), _outputs(want), tc.OUTPUTS, f"replay {k} vs composition")
        assert total > 0 and bool(scount.any())
