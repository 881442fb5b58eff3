"""GPU parity of remap / undistort / overlap_mask (unidepth_amd/remap.py -> ud_remap, ud_overlap_mask, csrc/remap.hip) against the numpy
fp32 restatement of tools/make_golden_remap.py, bit for bit on every point (neither kernel has a libm call); torch's CPU F.grid_sample, the
reference's own Camera.mask_overlap_projection and the reference's undistortion chain (tests/golden/remap.npz) at the measured bars; wave
and workgroup edges, both coordinate layouts, shared batches, guarded outputs, the camera classes' get_overlap_mask and graph replay.
Shared helpers: tests/remap_common.py.

Every case runs once per process through the C-ABI with guarded buffers, twice (_gpu_set), and is shared."""
import functools
import importlib

import numpy as np
import pytest
import torch

import layout_guard as lg
import remap_common as common

rm, gp = common.rm, common.gp
pytestmark = pytest.mark.gpu


def _guard(n, dtype):
    """`n` elements of `dtype` inside a guard allocation, seen as a flat tensor."""
    words = max(1, -(-n * torch.empty(0, dtype=dtype).element_size() // 4))
    g = lg.guarded(words, 1, 1, torch.float32)
    return g, g.view.reshape(-1).view(dtype)[:n]


def _t(a):
    """a numpy array as a C-contiguous host tensor of its own (the shared inputs are read-only)"""
    return torch.from_numpy(np.array(a, order="C"))


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _raw_remap(src, uv, cfg, mask=None, cv=None, out_u8=False, rows=True, want_valid=True, B=None):
    """ud_remap with out and valid inside sentinel-filled allocations, twice.  src numpy [B or 1,C,Hs,Ws], uv numpy [B or 1,N,2] handed
    over as rows or planes, mask [B or 1,Hs,Ws], cv [B,N].  Returns (out [B,N,C], valid bool [B,N] or None) on the host after checking
    the guards and that the two calls gave the same bits."""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    mode, padding, normalize, _, _ = cfg
    B = max(src.shape[0], uv.shape[0]) if B is None else B
    _, Cc, Hs, Ws = src.shape
    N = uv.shape[1]
    u8 = src.dtype == np.uint8
    if rows:
        dev_uv, strides = _t(uv).cuda(), (2 * N, 2, 1)
    else:
        dev_uv, strides = _t(uv.transpose(0, 2, 1)).cuda(), (2 * N, 1, N)
    if uv.shape[0] == 1:
        strides = (0,) + strides[1:]
    dev_src = _t(src).cuda()
    dev_mask = None if mask is None else _t(mask).cuda()
    dev_cv = None if cv is None else _t(cv).cuda()
    odt = torch.uint8 if out_u8 else torch.float32
    go, out = _guard(B * N * Cc, odt)
    gv, valid = _guard(B * N, torch.uint8)
    d = mk(_lib.UdRemap, src=dev_src, src_mask=dev_mask, uv=dev_uv, coord_valid=dev_cv, out=out.data_ptr(), valid=valid.data_ptr() if want_valid else None,
           batch_stride=strides[0], point_stride=strides[1], comp_stride=strides[2], n_points=N, B=B, C=Cc, Hs=Hs, Ws=Ws,
           mode=_lib.UD_REMAP_BILINEAR if mode == "bilinear" else _lib.UD_REMAP_NEAREST,
           padding=_lib.UD_REMAP_BORDER if padding == "border" else _lib.UD_REMAP_ZEROS, normalize=int(normalize), src_u8=int(u8), out_u8=int(out_u8),
           out_rows=int(rows), src_shared=int(src.shape[0] == 1), mask_shared=int(mask is not None and mask.shape[0] == 1))
    outs = []
    for _ in range(2):
        check(_lib.lib.ud_remap(d, cur_stream()), "ud_remap")
        torch.cuda.synchronize()
        outs.append((out.cpu().numpy().copy(), valid.cpu().numpy().copy()))
    lg.check_guards(go, gv)
    assert outs[0][0].tobytes() == outs[1][0].tobytes(), "two calls gave different bits"
    got = outs[0][0].reshape(B, N, Cc) if rows else np.ascontiguousarray(outs[0][0].reshape(B, Cc, N).transpose(0, 2, 1))
    if not want_valid:
        assert (gv.view.reshape(-1).view(torch.int32) == lg.SENTINEL[torch.float32]).all()       # an absent mask is not written
        return got, None
    assert np.array_equal(outs[0][1], outs[1][1]) and set(np.unique(outs[0][1])) <= {0, 1}
    return got, outs[0][1].reshape(B, N).astype(bool)


def _rows_for(cfg):
    return cfg[2] == cfg[3]                                     # both layouts get every mode and padding


@functools.lru_cache(maxsize=None)
def _gpu_set(name, cfg, out_u8=False, n=None, rows=None):
    d = common.inputs(name)
    n = d["uv"].shape[1] if n is None else n
    return _raw_remap(d["src"], d["uv"][:, :n], cfg, d["mask"] if cfg[3] else None, d["cv"][:, :n] if cfg[4] else None, out_u8,
                      _rows_for(cfg) if rows is None else rows, B=d["B"])


@pytest.mark.parametrize("name", list(common.SETS))
def test_sets_against_restatement(name):
    """every point of every set in all 32 configurations (both modes x both paddings x normalize x src_mask x coord_valid), the uint8
    output for the uint8 sources: bit-equal to the restatement, guards intact.  The sets hold regular points up to a quarter of the image
    outside it, NaN, +-inf, +-1e30, -0.0, exactly 0, exactly the size and one ulp beyond, exact half-integers and the rint ties."""
    u8 = common.inputs(name)["src"].dtype == np.uint8
    for cfg in common.CONFIGS:
        for out_u8 in ((False, True) if u8 else (False,)):
            got, valid = _gpu_set(name, cfg, out_u8)
            want, wvalid = common.want(name, cfg, out_u8)
            assert common.same_bits(got, want), (name, cfg, out_u8)
            assert np.array_equal(valid, wvalid), (name, cfg, out_u8)


@pytest.mark.parametrize("n", common.POINT_COUNTS)
def test_point_counts(n):
    """the first n points: 63 - 65 the wave's edge, 255 - 257 the workgroup's, both layouts"""
    name = "f32_37x53_c3_b3"
    for cfg in (("bilinear", "zeros", True, True, True), ("nearest", "border", False, False, True)):
        want, wvalid = common.want(name, cfg, False, n)
        for rows in (True, False):
            got, valid = _gpu_set(name, cfg, False, n, rows)
            assert common.same_bits(got, want) and np.array_equal(valid, wvalid), (n, cfg, rows)


def test_exact_pixel_centres_return_the_source_bits():
    """48 * 64 materialised centres (12 workgroups per image), a coordinate set shared by the batch: the source's bits in all four mode /
    padding pairs, every point valid"""
    for name in ("f32_48x64_c1_b3_shared_uv", "f32_37x53_c5_b1_centres"):
        d = common.inputs(name)
        src = d["src"]
        src_rows = np.ascontiguousarray(src.reshape(src.shape[0], src.shape[1], -1).transpose(0, 2, 1))
        for mode in rm.MODES:
            for padding in rm.PADDINGS:
                got, valid = _gpu_set(name, (mode, padding, False, False, False))
                assert np.array_equal(got.view(np.uint32), src_rows.view(np.uint32)) and valid.all(), (name, mode, padding)


def test_absent_valid_is_not_written_and_python_surface_gives_the_same_bits():
    module = importlib.import_module("unidepth_amd.remap")
    name = "f32_37x53_c3_b3"
    d = common.inputs(name)
    cfg = ("bilinear", "zeros", True, True, True)
    got, none = _raw_remap(d["src"], d["uv"], cfg, d["mask"], d["cv"], want_valid=False)
    assert none is None and common.same_bits(got, common.want(name, cfg)[0])
    for name in ("f32_37x53_c3_b3", "u8_37x53_c3_b3_shared_src", "u8_48x64_c5_b1", "f32_48x64_c1_b3_shared_uv"):
        d = common.inputs(name)
        src, uv, N = _t(d["src"]).cuda(), _t(d["uv"]).cuda(), d["uv"].shape[1]
        mask, cv = _t(d["mask"]).cuda(), _t(d["cv"]).cuda()
        for cfg in (("bilinear", "zeros", True, True, True), ("nearest", "border", False, False, False), ("bilinear", "border", False, True, False)):
            kw = dict(mode=cfg[0], padding=cfg[1], normalize=cfg[2], src_mask=mask[:, None].bool() if cfg[3] else None, coord_valid=cv.bool() if cfg[4] else None)
            want, wvalid = common.want(name, cfg, d["src"].dtype == np.uint8)
            out, valid = module.remap(src, uv, return_mask=True, **kw)
            assert out.shape == (d["B"], N, d["src"].shape[1]) and valid.shape == (d["B"], N) and valid.dtype == torch.bool
            assert common.same_bits(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wvalid), (name, cfg)
            n8 = N - N % 8                                       # the first n8 points as planes [B,2,8,n8/8]
            if n8:
                planes = uv[:, :n8].transpose(1, 2).reshape(uv.shape[0], 2, 8, n8 // 8)
                pkw = dict(kw, coord_valid=cv[:, :n8].reshape(-1, 1, 8, n8 // 8).bool()) if cfg[4] else kw
                out, valid = module.remap(src, planes, return_mask=True, **pkw)
                assert out.shape == (d["B"], d["src"].shape[1], 8, n8 // 8) and valid.shape == (d["B"], 1, 8, n8 // 8)
                assert common.same_bits(np.ascontiguousarray(out.reshape(d["B"], -1, n8).transpose(1, 2).cpu().numpy()), np.ascontiguousarray(want[:, :n8]))
                assert np.array_equal(valid.reshape(d["B"], n8).cpu().numpy(), wvalid[:, :n8])
            if d["src"].dtype == np.uint8:                       # fp32 out of a uint8 source; other float dtypes convert
                out = module.remap(src, uv, out_dtype=torch.float32, **kw)
                assert common.same_bits(out.cpu().numpy(), common.want(name, cfg, False)[0])
            else:
                assert torch.equal(_ibits(module.remap(src.double(), uv.double(), **kw)), _ibits(module.remap(src, uv, **kw)))


@pytest.mark.parametrize("name", list(rm.GS_CASES))
def test_against_grid_sample(name):
    """torch's CPU F.grid_sample (stored), both modes x both paddings, normalize off, no masks, every regular point: within
    max(4 e, 8 x 2^-24), e = grid_sample's own fp32 error against the fp64 restatement, |d| / max(|v|, 1), per mode"""
    g, bars = common.golden(), common.bars()
    src, uv = rm.gs_inputs(name)
    for mode in rm.MODES:
        for padding in rm.PADDINGS:
            cfg = (mode, padding, False, False, False)
            got, valid = _raw_remap(src, uv, cfg, rows=padding == "zeros")
            want, wvalid = rm.remap(src, uv, mode, padding)
            assert common.same_bits(got, want) and np.array_equal(valid, wvalid)
            r64 = rm.remap(src, uv, mode, padding, dtype=np.float64)[0]
            e = float(rm.value_error(got - g[f"{name}.{mode}.{padding}"], r64).max())
            print(f"{name} {mode} {padding}: vs grid_sample {e:.3e}, bar {bars[mode]:.3e}")
            assert e <= bars[mode], (name, mode, padding, e, bars[mode])
            size = np.array([src.shape[3], src.shape[2]])
            assert np.array_equal(valid, ((uv >= 0) & (uv <= size)).all(axis=2))


# ---- overlap mask ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gpu_overlap(name):
    """ud_overlap_mask with the mask inside a guard allocation, twice: bool [B,1,H,W] on the host"""
    from unidepth_amd import _lib
    from unidepth_amd.ops import check, cur_stream, mk
    uv = rm.nan_field() if name == "nan_37x53" else common.overlap_fields()[name]
    B, _, H, W = uv.shape
    dev = _t(uv).cuda()
    gm, mask = _guard(B * H * W, torch.uint8)
    d = mk(_lib.UdOverlapMask, uv=dev, mask=mask.data_ptr(), B=B, H=H, W=W)
    outs = []
    for _ in range(2):
        check(_lib.lib.ud_overlap_mask(d, cur_stream()), "ud_overlap_mask")
        torch.cuda.synchronize()
        outs.append(mask.cpu().numpy().copy())
    lg.check_guards(gm)
    assert np.array_equal(outs[0], outs[1]) and set(np.unique(outs[0])) <= {0, 1}
    return outs[0].reshape(B, 1, H, W).astype(bool)


def _overlap_names():
    return list(rm.OV_FIELDS) + ["proj_" + n for n in rm.OV_PROJECTED]


@pytest.mark.parametrize("name", _overlap_names() + ["nan_37x53"])
def test_overlap_mask_against_restatement(name):
    """every pixel, bit-equal; the NaN field is compared with the restatement only"""
    module = importlib.import_module("unidepth_amd.remap")
    uv = rm.nan_field() if name == "nan_37x53" else common.overlap_fields()[name]
    got = _gpu_overlap(name)
    assert np.array_equal(got, rm.overlap(uv)), name
    out = module.overlap_mask(torch.from_numpy(uv).cuda())
    assert out.dtype == torch.bool and out.shape == got.shape and np.array_equal(out.cpu().numpy(), got)
    assert np.array_equal(module.overlap_mask(torch.from_numpy(uv).cuda().double()).cpu().numpy(), got)


@pytest.mark.parametrize("name", _overlap_names())
def test_overlap_mask_against_reference(name):
    """the reference's own Camera.mask_overlap_projection on the CPU (stored): equal on every pixel the fp64 restatement keeps 1e-3 px
    from the decision that would change it; at most 1 % of a case's pixels is left out"""
    uv = common.overlap_fields()[name]
    margin = []
    m64 = rm.overlap(uv, np.float64, margin)
    keep = margin[0] >= rm.OVERLAP_MARGIN
    assert (~keep).reshape(uv.shape[0], -1).mean(axis=1).max() <= rm.BAND_CAP
    ref = common.unpack(common.golden()[name + ".overlap"], m64.shape)
    got = _gpu_overlap(name)
    assert np.array_equal(got[keep], ref[keep]), (name, int((got != ref)[keep].sum()))


def _mixed(name):
    """(BatchCamera, point maps [B,3,H,W] on the GPU, models) of a gt_points case; image b's points are those of image b + 1, so that the
    projection is not the identity"""
    from unidepth_amd import cameras, gtpoints
    depth, params, models = gp.case_rows(name)
    cam = gp.case_camera(cameras, name)
    pts = gtpoints.gt_points(torch.from_numpy(depth).cuda(), cam)
    return cam, torch.roll(pts, -1, 0).contiguous(), models


def test_camera_get_overlap_mask():
    """OPENCV and Fisheye624 set the mask of their uv; Pinhole, EUCM, Spherical and MEI set None; a BatchCamera with such a member gets
    [B,1,H,W] with all-True rows for the others, without one None; None before the first project(); what project() returned and stored
    before is unchanged: project_camera's own outputs"""
    from unidepth_amd import cameras, reproject
    module = importlib.import_module("unidepth_amd.remap")
    for name in ("mixed_5x7_b6", "mixed_37x53_b6"):
        batch, pts, models = _mixed(name)
        B = len(models)
        assert batch.get_overlap_mask() is None and all(c.get_overlap_mask() is None for c in batch.cameras)
        uv0, inside0, _ = reproject.project_camera(pts, batch)
        uv = batch.project(pts)
        assert torch.equal(_ibits(uv), _ibits(uv0))
        flip = torch.tensor([m == gp.PINHOLE for m in models]).cuda()[:, None, None, None]
        assert torch.equal(batch.get_projection_mask(), inside0[:, None] ^ flip)
        sets = [m in (gp.OPENCV, gp.FISHEYE624) for m in models]
        whole = module.overlap_mask(uv0)
        om = batch.get_overlap_mask()
        assert om.shape == (B, 1) + tuple(pts.shape[-2:]) and om.dtype == torch.bool
        for b, member in enumerate(batch.cameras):
            assert torch.equal(om[b], whole[b] if sets[b] else torch.ones_like(whole[b])), (name, b)
            one = member.project(pts[b:b + 1])
            assert torch.equal(_ibits(one), _ibits(uv0[b:b + 1]))
            pm = member.get_projection_mask()
            if models[b] == gp.SPHERICAL:
                assert pm is None
            else:
                assert torch.equal(pm, (inside0[b:b + 1, None] ^ flip[b:b + 1]))
            if sets[b]:
                assert torch.equal(member.get_overlap_mask(), whole[b:b + 1]), (name, b)
            else:
                assert member.get_overlap_mask() is None, (name, b)
        assert np.array_equal(whole.cpu().numpy(), rm.overlap(uv0.cpu().numpy()))
    # a BatchCamera without such a member: None, also after one with a member had set it on another object
    K = torch.tensor([[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]])
    plain = cameras.BatchCamera([cameras.Pinhole(K), cameras.EUCM(torch.tensor([50.0, 51, 26, 18, 0.5, 1.0]))])
    plain.project(pts[:2])
    assert plain.get_overlap_mask() is None and plain.get_projection_mask() is not None


# ---- undistort -----------------------------------------------------------------------------------------------------------------------

def _ud_cameras(name):
    from unidepth_amd import cameras
    src, params, models, dparams, dmodels = rm.ud_inputs(name)
    scam = cameras.BatchCamera([gp.make_camera(cameras, m, r) for m, r in zip(models, params)])
    dcam = None if rm.UD_CASES[name] is None else gp.make_camera(cameras, dmodels[0], dparams[0])
    return torch.from_numpy(src).cuda(), scam, dcam


@pytest.mark.parametrize("name", list(rm.UD_CASES))
def test_undistort_is_its_three_calls(name):
    """each of the six source models, the default Pinhole and an OPENCV destination: bit-equal to unproject_camera, project_camera and
    remap called one after the other; return_uv gives project_camera's uv; other modes and another output shape go the same way"""
    from unidepth_amd import gtpoints, reproject, unproject
    module = importlib.import_module("unidepth_amd.remap")
    src, scam, dcam = _ud_cameras(name)
    B, _, Hs, Ws = src.shape
    for kw, shape in ((dict(), None), (dict(mode="nearest", padding="border"), (20, 31)), (dict(normalize=True, src_mask=(src[:, :1] > 1.0)), (41, 50))):
        out, mask, uv = module.undistort(src, scam, dcam, shape, return_mask=True, return_uv=True, **kw)
        Ho, Wo = shape or (Hs, Ws)
        if dcam is None:
            rows = torch.zeros(B, 16, device="cuda")
            rows[:, :4] = gtpoints.prepare_camera(scam, B, "cuda").params[:, :4]
            dst = gtpoints.PreparedCamera(rows, (gp.PINHOLE,) * B)
        else:
            dst = gtpoints.prepare_camera(dcam, B, "cuda")
        rays = unproject.unproject_camera(None, dst, image_shape=(Ho, Wo))
        uv2, inside, depth = reproject.project_camera(rays, scam, image_shape=(Hs, Ws))
        out2, mask2 = module.remap(src, uv2, coord_valid=inside & (depth > 0), return_mask=True, **kw)
        assert out.shape == (B, src.shape[1], Ho, Wo) and mask.shape == (B, 1, Ho, Wo) and uv.shape == (B, 2, Ho, Wo)
        assert torch.equal(_ibits(uv), _ibits(uv2)) and torch.equal(_ibits(out), _ibits(out2)) and torch.equal(mask, mask2)
        assert torch.equal(_ibits(module.undistort(src, scam, dcam, shape, **kw)), _ibits(out))
        assert bool(mask.any())
    # one image, one camera of every model, the 1-camera form
    whole = module.undistort(src, scam, dcam)
    for b, member in enumerate(scam.cameras):
        one = module.undistort(src[b:b + 1], member, dcam)
        assert torch.equal(_ibits(one), _ibits(whole[b:b + 1])), (name, b)


@pytest.mark.parametrize("name", list(rm.UD_CASES))
def test_undistort_against_the_reference_chain(name):
    """grid_sample at src_cam.project(dst_cam.unproject(grid)) with the reference's own classes on the CPU (stored): masks equal and values
    within the measured bar on the pixels valid on both sides, outside the band (fp64 coordinate within 1e-2 px of the image border or of
    depth = 0; at most 1 % of a case)"""
    module = importlib.import_module("unidepth_amd.remap")
    g, bar = common.golden(), common.bars()["undistort"]
    src, scam, dcam = _ud_cameras(name)
    out, mask = module.undistort(src, scam, dcam, return_mask=True)
    B, Cc = src.shape[:2]
    got = np.ascontiguousarray(out.reshape(B, Cc, -1).transpose(1, 2).cpu().numpy())
    valid = mask.reshape(B, -1).cpu().numpy()
    uv64, _, o64, v64, d64 = rm.ud_chain(name, np.float64)
    keep = ~rm.ud_band(uv64, d64)
    assert (~keep).mean(axis=1).max() <= rm.BAND_CAP
    ref, rmask = g[name + ".out"], common.unpack(g[name + ".mask"], valid.shape)
    assert np.array_equal(valid[keep], rmask[keep]), (name, int((valid != rmask)[keep].sum()))
    both = keep & valid & rmask
    e = float(rm.value_error(got - ref, o64)[both].max())
    print(f"{name}: vs the reference's chain {e:.3e}, bar {bar:.3e}")
    assert both.mean() > 0.5 and e <= bar, (name, e, bar)


# ---- graph capture -----------------------------------------------------------------------------------------------------------------

def _captured(fn):
    """fn() captured once after a warm-up on a side stream: (graph, static output)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_graph_replay_after_inputs_were_overwritten():
    """remap and overlap_mask captured once, replayed after the coordinates and the source were overwritten in place: the replay equals
    a fresh call bit for bit"""
    module = importlib.import_module("unidepth_amd.remap")
    d = common.inputs("f32_37x53_c3_b3")
    src, uv = _t(d["src"]).cuda(), _t(d["uv"]).cuda()
    mask, cv = _t(d["mask"]).cuda()[:, None].bool(), _t(d["cv"]).cuda().bool()
    kw = dict(src_mask=mask, coord_valid=cv, normalize=True, return_mask=True)
    graph, (out, valid) = _captured(lambda: module.remap(src, uv, **kw))
    for k in range(3):
        src.copy_(torch.flip(src, (0, 3)) if k % 2 == 0 else src * 0.5)
        uv.copy_(torch.flip(uv, (1,)) if k % 2 == 0 else uv + 0.37)
        graph.replay()
        torch.cuda.synchronize()
        fresh, fvalid = module.remap(src, uv, **kw)
        assert torch.equal(_ibits(out), _ibits(fresh)) and torch.equal(valid, fvalid), f"replay {k}"
        want, wvalid = rm.remap(src.cpu().numpy(), uv.cpu().numpy(), "bilinear", "zeros", d["mask"], d["cv"], True)
        assert common.same_bits(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wvalid), f"replay {k}"
    field = torch.from_numpy(rm.overlap_field("barrel_37x53")).cuda()
    graph, om = _captured(lambda: module.overlap_mask(field))
    for other in ("fold_37x53", "mild_37x53"):
        field.copy_(torch.from_numpy(rm.overlap_field(other)).cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(om, module.overlap_mask(field)) and np.array_equal(om.cpu().numpy(), rm.overlap(rm.overlap_field(other))), other
