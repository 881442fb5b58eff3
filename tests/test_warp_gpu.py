"""GPU parity of warp_camera (unidepth_amd/warp.py -> ud_warp_camera, csrc/warp.hip) against the composition of the already merged calls
-- unproject_camera, project_camera, remap, remap of the source's depth and the comparison (tests/warp_common.py oracle) -- bit for bit in
every output at every pixel, compared as integers: both sides inline the same functions of camera_models.h and remap_taps.h under
-ffp-contract=off.  Every output of the fused call sits inside a guarded allocation (tests/layout_guard.py), the uint8 ones at an odd
byte offset."""
import functools

import numpy as np
import pytest
import torch

import layout_guard as lg
import warp_common as wc

pytestmark = pytest.mark.gpu
_SENTINEL_BYTES = (0xAD, 0xDB, 0xBA, 0x7F)                     # lg.SENTINEL[torch.float32], little endian


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

    def check(self, name, written=True):
        self.g.check_guards(name)
        want = torch.tensor(_SENTINEL_BYTES, dtype=torch.uint8, device="cuda").repeat(self.words)
        keep = torch.ones_like(want, dtype=torch.bool)
        if written:
            keep[self.lo:self.hi] = False
        assert torch.equal(self.bytes[keep], want[keep]), f"{name}: bytes beside the output were rewritten" if written else f"{name}: an absent output was written"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    return t if dtype is None else t.to(dtype)


def _raw_warp(src, *, depth=None, points=None, cam_d=None, cam_s, T=None, mode="bilinear", padding="zeros", src_mask=None, valid_in=None,
              normalize=False, out_dtype=None, src_depth=None, tol=0.0, want=("valid", "visible", "uv", "proj_depth")):
    """ud_warp_camera through the C-ABI on device tensors, every output inside a guarded allocation (absent ones too: they must stay
    untouched), twice.  -> (out, valid bool [B,1,Ho,Wo], visible bool [B,1,Ho,Wo] or None, uv, proj_depth) in the oracle's shapes"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    geo = depth if depth is not None else points
    Bn, (Ho, Wo) = geo.shape[0], geo.shape[-2:]
    sb, Cc, Hs, Ws = src.shape
    n = Ho * Wo
    u8 = src.dtype == torch.uint8
    out_dtype = out_dtype or (torch.uint8 if u8 else torch.float32)
    o8 = out_dtype == torch.uint8
    bufs = dict(out=_Out(Bn * Cc * n, out_dtype, 1 if o8 else 0), valid=_Out(Bn * n, torch.uint8, 3), visible=_Out(Bn * n, torch.uint8, 1),
                uv=_Out(Bn * 2 * n, torch.float32), proj_depth=_Out(Bn * n, torch.float32, 1))
    has = {k: k == "out" or (k in want and (k != "visible" or src_depth is not None)) for k in bufs}
    d = mk(_lib.UdWarpCamera, src=src.contiguous(), src_mask=None if src_mask is None else src_mask.contiguous().view(torch.uint8),
           src_depth=None if src_depth is None else src_depth.contiguous(), points=None if points is None else points.contiguous(),
           depth=None if depth is None else depth.contiguous(), params_dst=None if cam_d is None else cam_d.params, params_src=cam_s.params,
           T=None if T is None else T.contiguous(), valid_in=None if valid_in is None else valid_in.contiguous().view(torch.uint8),
           B=Bn, C=Cc, Ho=Ho, Wo=Wo, Hs=Hs, Ws=Ws, nT=0 if T is None else T.shape[0], mode=wc.MODES[mode], padding=wc.PADDINGS[padding],
           normalize=int(normalize), src_u8=int(u8), out_u8=int(o8), src_shared=int(sb == 1), mask_shared=int(src_mask is not None and src_mask.shape[0] == 1),
           depth_shared=int(src_depth is not None and src_depth.shape[0] == 1), tol_bits=wc.tol_bits(tol),
           **{k: (b.t.data_ptr() if has[k] else None) for k, b in bufs.items()})
    for b in range(Bn):
        d.model_src[b] = cam_s.models[b]
        if cam_d is not None:
            d.model_dst[b] = cam_d.models[b]
    runs = []
    for _ in range(2):
        check(_lib.lib.ud_warp_camera(d, cur_stream()), "ud_warp_camera")
        torch.cuda.synchronize()
        runs.append({k: b.t.clone() for k, b in bufs.items() if has[k]})
    for k, b in bufs.items():
        b.check(k, has[k])
    for k in runs[0]:
        assert torch.equal(wc.bits(runs[0][k]), wc.bits(runs[1][k])), f"two calls gave different bits in {k}"
    r = runs[0]
    for k in ("valid", "visible"):
        if k in r:
            assert int(r[k].max()) <= 1
    return (r["out"].view(Bn, Cc, Ho, Wo), r["valid"].view(Bn, 1, Ho, Wo).bool() if "valid" in r else None,
            r["visible"].view(Bn, 1, Ho, Wo).bool() if "visible" in r else None, r["uv"].view(Bn, 2, Ho, Wo) if "uv" in r else None,
            r["proj_depth"].view(Bn, Ho, Wo) if "proj_depth" in r else None)


@functools.lru_cache(maxsize=None)
def _device_case(name, Ho=wc.HO, Wo=wc.WO, Hs=wc.HS, Ws=wc.WS):
    """a case of warp_common on the GPU (shared, never written): tensors, and both cameras as PreparedCamera"""
    c = wc.case(name, Ho, Wo, Hs, Ws)
    d = {k: _dev(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    d["cam_d"], d["cam_s"] = wc.prepared(c["params_dst"], c["models_dst"]), wc.prepared(c["params_src"], c["models_src"])
    return d


def _source(d, kind):
    dt, _, odt, has_mask, normalize = wc.KINDS[kind]
    return (d["src_f32"] if dt == np.float32 else d["src_u8"]), (d["src_mask"] if has_mask else None), normalize, (torch.uint8 if odt == np.uint8 else torch.float32)


def _transform(d, which):
    return {"none": None, "shared": d["T_shared"][None], "batch": d["T_batch"]}[which]


@pytest.mark.parametrize("name", [n for n in wc.DST_SETS if n != "iterative"])
def test_matrix_against_the_composition(name):
    """each closed-form destination model against a source batch of all six models, and a mixed destination batch; both modes x both
    paddings x {fp32 C = 1 with mask, normalised; uint8 C = 3 -> uint8; uint8 -> fp32} x {no, a shared, a per-image transform}; all optional
    outputs on, every output guarded.  At least a quarter of every image's pixels is valid and at least a tenth is not (the shares were
    checked on the host program first, tests/test_warp_cpu.py asserts them too), so no case passes on an empty comparison."""
    d = _device_case(name)
    some_visible = False
    for tr in wc.TRANSFORMS:
        T = _transform(d, tr)
        for kind in wc.KINDS:
            src, mask, norm, odt = _source(d, kind)
            for mode in wc.MODES:
                for pad in wc.PADDINGS:
                    kw = dict(mode=mode, padding=pad, src_mask=mask, valid_in=d["valid_in"], normalize=norm, out_dtype=odt, src_depth=d["src_depth"])
                    got = _raw_warp(src, depth=d["depth"], cam_d=d["cam_d"], cam_s=d["cam_s"], T=T, tol=wc.TOL, **kw)
                    want = wc.oracle(src, depth=d["depth"], camera=d["cam_d"], src_camera=d["cam_s"], transform=T, occlusion_tol=wc.TOL, **kw)
                    wc.assert_same(got, want, f"{name} {tr} {kind} {mode} {pad}")
                    share = got[1].reshape(wc.B, -1).float().mean(dim=1)
                    assert float(share.min()) >= 0.25 and float(share.max()) <= 0.9, (name, tr, kind, mode, pad, share.tolist())
                    some_visible = some_visible or (bool(got[2].any()) and not bool(got[2][got[1]].all()))
    assert some_visible


def test_python_surface_gives_the_same_bits():
    """warp_camera() itself: the raw call's bits, the order and shapes of what it returns, a tuple only for more than one result; camera
    objects and prepared cameras, depth as [B,1,H,W] or [B,H,W], a [4,4] transform, shared source maps, other float dtypes converted"""
    import remap_common
    from unidepth_amd import cameras, warp
    gp = remap_common.gp
    d, c = _device_case("mixed"), wc.case("mixed")
    cam_d = cameras.BatchCamera([gp.make_camera(cameras, m, r) for m, r in zip(c["models_dst"], c["params_dst"])])
    cam_s = cameras.BatchCamera([gp.make_camera(cameras, m, r) for m, r in zip(c["models_src"], c["params_src"])])
    T44 = torch.eye(4, device="cuda").repeat(wc.B, 1, 1)
    T44[:, :3] = d["T_batch"]
    for kind, mode, pad in (("f32_c1_mask_norm", "bilinear", "zeros"), ("u8_c3", "nearest", "border"), ("u8_c3_f32", "bilinear", "border")):
        src, mask, norm, odt = _source(d, kind)
        kw = dict(mode=mode, padding=pad, src_mask=mask, valid_in=d["valid_in"], normalize=norm, out_dtype=odt)
        raw = _raw_warp(src, depth=d["depth"], cam_d=d["cam_d"], cam_s=d["cam_s"], T=d["T_batch"], src_depth=d["src_depth"], tol=wc.TOL, **kw)
        res = warp.warp_camera(src, depth=d["depth"], camera=cam_d, src_camera=cam_s, transform=T44, src_depth=d["src_depth"], occlusion_tol=wc.TOL,
                               return_mask=True, return_uv=True, return_depth=True, **kw)
        assert isinstance(res, tuple) and len(res) == 5 and res[1].dtype == res[2].dtype == torch.bool
        wc.assert_same(res, raw, f"wrapper {kind}")
        res = warp.warp_camera(src, depth=d["depth"][:, 0], camera=d["cam_d"], src_camera=d["cam_s"], transform=d["T_batch"], return_depth=True, **kw)
        assert len(res) == 2 and torch.equal(wc.bits(res[0]), wc.bits(raw[0])) and torch.equal(wc.bits(res[1]), wc.bits(raw[4]))
        one = warp.warp_camera(src, depth=d["depth"], camera=d["cam_d"], src_camera=d["cam_s"], transform=d["T_batch"], **kw)
        assert isinstance(one, torch.Tensor) and torch.equal(wc.bits(one), wc.bits(raw[0]))
        out, visible = warp.warp_camera(src, depth=d["depth"], camera=d["cam_d"], src_camera=d["cam_s"], transform=d["T_batch"], src_depth=d["src_depth"],
                                        occlusion_tol=wc.TOL, **kw)
        assert torch.equal(visible, raw[2])
    src, mask, norm, odt = _source(d, "f32_c1_mask_norm")
    kw = dict(depth=d["depth"], camera=d["cam_d"], src_camera=d["cam_s"], src_mask=mask, normalize=True, return_mask=True)
    a = warp.warp_camera(src.double(), src_depth=d["src_depth"].double(), occlusion_tol=wc.TOL, **kw)
    b = warp.warp_camera(src, src_depth=d["src_depth"], occlusion_tol=wc.TOL, **kw)
    assert all(torch.equal(wc.bits(x), wc.bits(y)) for x, y in zip(a, b))


def test_iterative_destinations_through_the_points_path():
    """OPENCV and Fisheye624 destination members: the wrapper unprojects the whole batch first and ANDs depth > 0 into valid_in; equal to
    the composition, with and without a valid_in of the caller's; the entry point itself refuses them"""
    from unidepth_amd import warp
    d = _device_case("iterative")
    for kind, mode, pad, tr, vin in (("f32_c1_mask_norm", "bilinear", "zeros", "batch", True), ("u8_c3", "nearest", "border", "shared", False),
                                     ("u8_c3_f32", "bilinear", "border", "none", True), ("u8_c3", "bilinear", "zeros", "batch", False)):
        src, mask, norm, odt = _source(d, kind)
        kw = dict(depth=d["depth"], camera=d["cam_d"], src_camera=d["cam_s"], transform=_transform(d, tr), mode=mode, padding=pad, src_mask=mask,
                  valid_in=d["valid_in"] if vin else None, normalize=norm, out_dtype=odt, src_depth=d["src_depth"], occlusion_tol=wc.TOL)
        got = warp.warp_camera(src, return_mask=True, return_uv=True, return_depth=True, **kw)
        want = wc.oracle(src, **kw)
        wc.assert_same(got, want, f"iterative {kind} {mode} {pad} {tr}")
        share = got[1].reshape(wc.B, -1).float().mean(dim=1)
        assert float(share.min()) >= 0.25 and float(share.max()) <= 0.9, share.tolist()
    with pytest.raises(RuntimeError, match="iterative destination"):
        _raw_warp(d["src_f32"], depth=d["depth"], cam_d=d["cam_d"], cam_s=d["cam_s"])


@pytest.mark.parametrize("model", wc.CLOSED)
def test_front_ends_agree(model):
    """the points of unproject_camera with valid_in = depth > 0 give the bits of the depth form, in every output"""
    from unidepth_amd import unproject, warp
    d = _device_case(wc.NAMES[model])
    src, mask, norm, odt = _source(d, "f32_c1_mask_norm")
    kw = dict(src_camera=d["cam_s"], transform=d["T_batch"], src_mask=mask, normalize=norm, src_depth=d["src_depth"], occlusion_tol=wc.TOL,
              return_mask=True, return_uv=True, return_depth=True)
    a = warp.warp_camera(src, depth=d["depth"], camera=d["cam_d"], **kw)
    pts = unproject.unproject_camera(None, d["cam_d"], depth=d["depth"], image_shape=(wc.HO, wc.WO))
    b = warp.warp_camera(src, points=pts, valid_in=d["depth"] > 0, **kw)
    wc.assert_same(a, b, f"front ends {wc.NAMES[model]}")
    assert bool(a[1].any()) and not bool(a[1].all())


def test_special_values():
    """destination depth 0, negative, NaN, +-inf, -0.0; transforms with 1e30 entries, to z' = 0 and to z' < 0; NaN and 0 in src_depth: out
    is 0 and valid / visible are 0 exactly where the composition says (and on the pixels known to be dead), nothing else differs"""
    c, depth, T, sd = wc.special_case()
    depth, T, sd = _dev(depth), _dev(T), _dev(sd)
    dead = torch.zeros(wc.B, 1, wc.HO, wc.WO, dtype=torch.bool, device="cuda")
    dead[:, :, 0, 0:4] = True
    dead[:, :, 1, 0:3] = True
    dead[3:5] = True
    for name in ("mixed", "pinhole", "spherical"):
        d = _device_case(name)
        for kind, mode, pad in (("f32_c1_mask_norm", "bilinear", "zeros"), ("u8_c3", "nearest", "border"), ("u8_c3_f32", "bilinear", "border"),
                                ("f32_c1_mask_norm", "nearest", "zeros")):
            src, mask, norm, odt = _source(_device_case("mixed"), kind)
            kw = dict(mode=mode, padding=pad, src_mask=mask, normalize=norm, out_dtype=odt, src_depth=sd)
            got = _raw_warp(src, depth=depth, cam_d=d["cam_d"], cam_s=d["cam_s"], T=T, tol=wc.TOL, **kw)
            want = wc.oracle(src, depth=depth, camera=d["cam_d"], src_camera=d["cam_s"], transform=T, occlusion_tol=wc.TOL, **kw)
            wc.assert_same(got, want, f"special {name} {kind} {mode} {pad}")
            assert not bool(got[1][dead].any()) and not bool(got[2][dead].any()) and not bool(got[0][dead.expand_as(got[0])].any())
            assert bool(got[1][0].any()) and bool(got[1][5].any())
    # the points form: z' = 0 and z' < 0 in the points themselves, no transform
    d = _device_case("mixed")
    pts = _dev(wc.points_in_front(np.random.RandomState(9201), wc.B, wc.HO, wc.WO))
    got = _raw_warp(d["src_u8"], points=pts, cam_s=d["cam_s"], src_depth=sd, tol=wc.TOL)
    want = wc.oracle(d["src_u8"], points=pts, src_camera=d["cam_s"], src_depth=sd, occlusion_tol=wc.TOL)
    wc.assert_same(got, want, "special points")
    behind = (pts[:, 2:3] <= 0)
    assert float(behind.float().mean()) > 0.1 and not bool(got[1][behind].any()) and not bool(got[0][behind.expand_as(got[0])].any())


@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257))
def test_destination_pixel_counts(n):
    """H = 1 and 1 .. 257 pixels: the wave's and the workgroup's edges; only `out` asked for: the other four outputs stay untouched"""
    d = _device_case("mixed", 1, n)
    rows_d = d["cam_d"].params.clone()
    rows_d[:, 2], rows_d[:, 3] = n / 2, 0.5                                    # the single row looks along the axis
    cam_d = wc.prepared(rows_d.cpu().numpy(), d["cam_d"].models)
    for kind, mode, pad in (("f32_c1_mask_norm", "bilinear", "zeros"), ("u8_c3", "nearest", "border")):
        src, mask, norm, odt = _source(d, kind)
        kw = dict(mode=mode, padding=pad, src_mask=mask, valid_in=d["valid_in"], normalize=norm, out_dtype=odt, src_depth=d["src_depth"])
        got = _raw_warp(src, depth=d["depth"], cam_d=cam_d, cam_s=d["cam_s"], T=d["T_batch"], tol=wc.TOL, **kw)
        want = wc.oracle(src, depth=d["depth"], camera=cam_d, src_camera=d["cam_s"], transform=d["T_batch"], occlusion_tol=wc.TOL, **kw)
        wc.assert_same(got, want, f"n = {n} {kind}")
        assert n < 63 or bool(got[1].any())
        only = _raw_warp(src, depth=d["depth"], cam_d=cam_d, cam_s=d["cam_s"], T=d["T_batch"], tol=wc.TOL, want=(), **kw)
        assert torch.equal(wc.bits(only[0]), wc.bits(got[0])) and only[1:] == (None, None, None, None)


@pytest.mark.parametrize("size", ((1, 1), (2, 3)))
def test_tiny_and_shared_sources(size):
    """sources of 1x1 and 2x3 pixels; src, src_mask and src_depth shared by the batch"""
    Hs, Ws = size
    d = _device_case("mixed", wc.HO, wc.WO, Hs, Ws)
    rows_s = d["cam_s"].params.clone()
    rows_s[:, 0], rows_s[:, 1], rows_s[:, 2], rows_s[:, 3] = 2.0 * Ws, 2.0 * Hs, Ws / 2, Hs / 2
    rows_s[2, 4], rows_s[2, 5] = Ws + 1.0, Hs + 1.0                            # Spherical's own W, H (W - 1 divides)
    rows_s[5, 0], rows_s[5, 1] = 4.0 * Ws, 4.0 * Hs                            # MEI: xi = 0.9 nearly halves the focal length
    cam_s = wc.prepared(rows_s.cpu().numpy(), d["cam_s"].models)
    valid_seen = False
    for shared in (False, True):
        pick = (lambda t: t[:1]) if shared else (lambda t: t)
        for kind, mode, pad in (("f32_c1_mask_norm", "bilinear", "zeros"), ("u8_c3", "nearest", "border"), ("u8_c3_f32", "bilinear", "border"),
                                ("u8_c3", "nearest", "zeros")):
            src, mask, norm, odt = _source(d, kind)
            kw = dict(mode=mode, padding=pad, src_mask=None if mask is None else pick(mask), valid_in=d["valid_in"], normalize=norm, out_dtype=odt,
                      src_depth=pick(d["src_depth"]))
            got = _raw_warp(pick(src), depth=d["depth"], cam_d=d["cam_d"], cam_s=cam_s, T=d["T_shared"][None], tol=wc.TOL, **kw)
            want = wc.oracle(pick(src), depth=d["depth"], camera=d["cam_d"], src_camera=cam_s, transform=d["T_shared"][None], occlusion_tol=wc.TOL, **kw)
            wc.assert_same(got, want, f"source {Hs}x{Ws} shared={shared} {kind} {mode} {pad}")
            valid_seen = valid_seen or bool(got[1].any())
    assert valid_seen


def test_known_answer():
    """fx = fy = 64, cx = 32, cy = 16, depth 2, translation (0.5, 0, 0): out[..., x] == src[..., x + 16], exact in fp32; translation 0
    returns src; src_depth 2 is visible wherever valid, 3 with a tolerance of 0.25 nowhere"""
    from unidepth_amd import warp
    k = wc.known_answer_inputs()
    cam = wc.prepared(k["rows"], (wc.PINHOLE,) * k["B"])
    src, depth = _dev(k["src"]), _dev(k["depth"])

    def run(T, sd, mode):
        kw = {} if sd is None else dict(src_depth=_dev(sd), occlusion_tol=wc.TOL)
        res = warp.warp_camera(src, depth=depth, camera=cam, src_camera=cam, transform=_dev(T), mode=mode, return_mask=True, **kw)
        return res[0].cpu().numpy(), res[1][:, 0].cpu().numpy(), (res[2][:, 0].cpu().numpy() if sd is not None else None)
    wc.check_known_answer(run)


def test_graph_replay_after_inputs_were_rewritten():
    """captured once; replayed after the depth buffer, the transform buffer and both cameras' parameter rows were rewritten in place:
    each replay equals the eager call and the composition"""
    from unidepth_amd import gtpoints, warp
    d, e = _device_case("mixed"), _device_case("eucm")
    depth, T = d["depth"].clone(), d["T_batch"].clone()
    cam_d = gtpoints.PreparedCamera(d["cam_d"].params.clone(), d["cam_d"].models)
    cam_s = gtpoints.PreparedCamera(d["cam_s"].params.clone(), d["cam_s"].models)
    kw = dict(depth=depth, camera=cam_d, src_camera=cam_s, transform=T, src_mask=d["src_mask"], valid_in=d["valid_in"], normalize=True,
              src_depth=d["src_depth"], occlusion_tol=wc.TOL)
    fn = lambda: warp.warp_camera(d["src_f32"], return_mask=True, return_uv=True, return_depth=True, **kw)       # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    for k in range(3):
        depth.copy_(e["depth"] if k % 2 == 0 else torch.flip(depth, (0, 3)))
        T.copy_(torch.flip(d["T_batch"], (0,)) if k % 2 == 0 else e["T_batch"])
        cam_d.params.mul_(1.03 if k % 2 == 0 else 0.95)
        cam_s.params[:, :2].mul_(0.9 if k % 2 == 0 else 1.07)
        graph.replay()
        torch.cuda.synchronize()
        wc.assert_same(static, fn(), f"replay {k} vs eager")
        wc.assert_same(static, wc.oracle(d["src_f32"], **kw), f"replay {k} vs composition")
        assert bool(static[1].any())
