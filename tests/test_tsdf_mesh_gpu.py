"""GPU parity of tsdf_mesh (unidepth_amd/tsdfmesh.py -> ud_tsdf_mesh, csrc/tsdf_mesh.hip) against the numpy fp32 restatement of
tests/tsdf_mesh_common.py, bit for bit in every output -- vertices, colours, normals, faces, counts and offsets -- compared as integers.
The scenes are those tests/test_tsdf_mesh_cpu.py checks on the host build of the same header; the grids walk round the 1024-item tile of
csrc/compact.h; the raw C-ABI calls write into guarded allocations (tests/layout_guard.py) at odd offsets with a dirty workspace."""
import numpy as np
import pytest
import torch

import layout_guard as lg
import tsdf_common as tc
import tsdf_mesh_common as mc

pytestmark = pytest.mark.gpu
_SENTINEL_BYTES = (0xAD, 0xDB, 0xBA, 0x7F)                     # lg.SENTINEL[torch.float32], little endian
KEYS = ("vertices", "faces", "rgb", "normals", "vert_counts", "vert_offsets", "face_counts", "face_offsets")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _volume(s, color=True):
    from unidepth_amd import tsdf
    return tsdf.TsdfVolume(_dev(s["tsdf"]), _dev(s["weight"]), _dev(s["color"]) if color and s.get("color") is not None else None,
                           _dev(s["origin"]), s["voxel"])


def _as_tuple(m):
    return tuple(getattr(m, k) for k in KEYS)


def _want(p, rgb=True, normals=True):
    return tuple(None if (p[k] is None or (k == "rgb" and not rgb) or (k == "normals" and not normals)) else _dev(p[k]) for k in KEYS)


def _check(s, what, min_weight=1.0):
    """tsdf_mesh on the volume s in every form of its optional outputs against the restatement -> the restatement's packed dict"""
    from unidepth_amd import tsdfmesh
    r = mc.cells(s["tsdf"], s["weight"], s.get("color"), s["origin"], s["voxel"], min_weight)
    p8, pf = mc.packed(r, rgb_u8=True), mc.packed(r, rgb_u8=False)
    vol = _volume(s)
    same = tc.host_program.assert_same
    same(_as_tuple(tsdfmesh.tsdf_mesh(vol, min_weight=min_weight, return_normals=True)), _want(p8), KEYS, what + " u8 normals")
    same(_as_tuple(vol.mesh(min_weight=min_weight, rgb_dtype=torch.float32)), _want(pf, normals=False), KEYS, what + " f32")
    if vol.color is not None:
        same(_as_tuple(tsdfmesh.tsdf_mesh(_volume(s, color=False), min_weight=min_weight)), _want(p8, rgb=False, normals=False), KEYS, what + " plain")
    return p8


def _field(grid, seed, B=1):
    """a normal field with a few NaN and a few voxels without weight: nearly every cell has a sign change, and some are dead"""
    g = np.random.RandomState(5200 + seed)
    t = g.normal(size=(B,) + tuple(grid)).astype(np.float32)
    t[g.uniform(size=t.shape) < 0.01] = np.nan
    w = (g.uniform(size=t.shape) >= 0.03).astype(np.float32) * 2
    return dict(tsdf=t, weight=w, color=g.uniform(0, 255, size=(B, 3) + tuple(grid)).astype(np.float32),
                origin=g.uniform(-1, 1, size=(B, 3)).astype(np.float32), voxel=tc.f32(0.05))


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.SCENES)
def test_scenes(name):
    p = _check(mc.scene(name), name)
    assert len(p["vertices"]) == int(mc.restated(name)["live"].sum()) > 0 and len(p["faces"]) > 0


def test_integrated_volume_with_colours():
    """a volume made by tsdf_integrate at 9 x 13 x 21 from three mixed views with colours and weights, two images"""
    from unidepth_amd import tsdf
    d = tc.scene(tc.mixed_models(), **tc.BASE)
    cams = [tc.prepared(d["params"][v], d["models"][v]) for v in range(d["V"])]
    vol = tsdf.tsdf_integrate(None, _dev(d["depths"]), cams, _dev(d["T"]), grid_shape=d["grid"], origin=_dev(d["origin"]), voxel_size=d["voxel"],
                              trunc=d["trunc"], src_weights=_dev(d["src_weights"]), images=_dev(d["images"]))
    s = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=vol.color.cpu().numpy(), origin=vol.origin.cpu().numpy(), voxel=vol.voxel_size)
    for mw in (1.0, 0.6):
        p = _check(s, f"integrated min_weight={mw}", min_weight=mw)
        assert (p["vert_counts"] > 50).all() and (p["face_counts"] > 50).all(), p["vert_counts"]


@pytest.mark.parametrize("per_origin", (False, True))
def test_batch_with_an_empty_middle_member(per_origin):
    s = mc.batch(("special", "sphere", "hole"), per_origin=per_origin)
    s["weight"] = s["weight"].copy()
    s["weight"][1] = 0
    p = _check(s, f"batch per_origin={per_origin}")
    assert p["vert_counts"].tolist() == [196, 0, 98] and p["face_counts"][1] == 0 and p["face_offsets"][1] == p["face_offsets"][2]
    assert int(p["faces"][p["face_offsets"][2]:].max()) < 98                      # rows local to the volume


# ---- around the tile ------------------------------------------------------------------------------------------------------------------

# (Nz, Ny, Nx): 1023, 1026, 2049 and 2050 voxels around the tile of 1024 cells (2049 = 3 * 683 has no grid with cells: an empty mesh over
# three tiles); rows of 63, 64, 65 and 257 voxels around the wave and the workgroup; 9 x 35 x 40 = 12,600 voxels: 13 cell tiles, 37 slot tiles
TILE_GRIDS = ((3, 11, 31), (3, 18, 19), (3, 683, 1), (2, 25, 41), (3, 3, 63), (3, 3, 64), (3, 3, 65), (2, 3, 257), (9, 35, 40))


@pytest.mark.parametrize("grid", TILE_GRIDS, ids=lambda g: "x".join(str(k) for k in g))
def test_grids_around_the_tile(grid):
    s = _field(grid, grid[2], B=2)
    p = _check(s, str(grid))
    if min(grid) > 1:
        cells = 2 * (grid[0] - 1) * (grid[1] - 1) * (grid[2] - 1)
        assert 0.3 * cells < len(p["vertices"]) < cells and len(p["faces"]) > 0, (len(p["vertices"]), cells)
    else:
        assert len(p["vertices"]) == 0 and len(p["faces"]) == 0


def test_more_than_256_slot_tiles():
    """16 x 10 x 683 voxels: 107 cell tiles and 321 slot tiles per volume, so the scan of a volume's quad counts takes a second chunk
    with the carry of the first; quads on both sides of tile 256, asserted on the restatement"""
    s = _field((16, 10, 683), 257)
    r = mc.cells(s["tsdf"], s["weight"], None, s["origin"], s["voxel"], 1.0)
    per_tile = np.add.reduceat(r["quad_live"][0], np.arange(0, r["quad_live"].shape[1], 1024))
    assert per_tile.shape == (321,) and (per_tile[[255, 256, 257, 290]] > 0).all()
    _check(dict(s, color=None), "321 slot tiles")


def test_quads_across_tiles_and_inside_one_word():
    """the plane between the z layers 0 and 1.  (3, 33, 32): rows of 32 cells, so the four cells of a quad lie in different words and, where
    a row of the grid ends a tile, in different tiles (992 vertices, 930 quads).  (3, 5, 7): all 24 cells in one word"""
    from unidepth_amd import tsdfmesh
    for grid, nv, nq in (((3, 33, 32), 992, 930), ((3, 5, 7), 24, 15)):
        for below_positive in (True, False):
            t, w = mc.plane(grid, below_positive)
            s = dict(tsdf=t, weight=w, color=None, origin=np.zeros((1, 3), np.float32), voxel=tc.f32(0.25))
            p = _check(s, f"plane {grid}")
            assert len(p["vertices"]) == nv and len(p["quads"]) == nq
            m = tsdfmesh.tsdf_mesh(_volume(s))
            assert m.vertices.shape == (nv, 3) and m.faces.shape == (2 * nq, 3) and m.rgb is None and m.normals is None
            if grid == (3, 5, 7):
                assert m.faces[:2].tolist() == ([[0, 6, 7], [0, 7, 1]] if below_positive else [[0, 1, 7], [0, 7, 6]])


# ---- capacities and empty results ---------------------------------------------------------------------------------------------------

def test_min_weight_above_every_weight_gives_an_empty_mesh():
    from unidepth_amd import tsdfmesh
    vol = _volume(mc.batch(("sphere", "pair")))
    for kw in ({}, dict(vert_capacity=7, face_capacity=5), dict(vert_capacity=0, face_capacity=0)):
        m = tsdfmesh.tsdf_mesh(vol, min_weight=1.5, return_normals=True, **kw)
        for c in (m.vert_counts, m.vert_offsets, m.face_counts, m.face_offsets):
            assert not bool(c.any())
        assert m.vertices.shape == (kw.get("vert_capacity", 0), 3) and m.faces.shape == (kw.get("face_capacity", 0), 3)
        assert m.rgb.shape == m.vertices.shape and m.normals.shape == m.vertices.shape and m.rgb.dtype == torch.uint8


def test_capacities_given_equal_counted():
    from unidepth_amd import _lib, tsdfmesh
    s = mc.batch(("sphere", "hole", "pair"), per_origin=True)
    vol = _volume(s)
    full = tsdfmesh.tsdf_mesh(vol, return_normals=True)
    nv, nf = full.vertices.shape[0], full.faces.shape[0]
    assert (nv, nf) == (180 + 98 + 140, 356 + 82 + 272)
    need = int(_lib.lib.ud_tsdf_mesh_work_bytes(3, 9, 13, 11))
    work = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    given = tsdfmesh.tsdf_mesh(vol, return_normals=True, vert_capacity=nv, face_capacity=nf, workspace=work)
    tc.host_program.assert_same(_as_tuple(given), _as_tuple(full), KEYS, "capacities given")
    assert bool((work[need:] == 0xFF).all())
    big = tsdfmesh.tsdf_mesh(vol, return_normals=True, vert_capacity=nv + 9, face_capacity=nf + 3)
    tc.host_program.assert_same((big.vertices[:nv], big.faces[:nf], big.rgb[:nv], big.normals[:nv]) + _as_tuple(big)[4:],
                                _as_tuple(full), KEYS, "capacities above the totals")
    # below the totals: the rows that fit are the same, the totals stay true; an odd face capacity holds no half quad (checked on guarded
    # memory in test_guarded_mesh)
    part = tsdfmesh.tsdf_mesh(vol, return_normals=True, vert_capacity=nv - 11, face_capacity=nf - 7)
    whole = (nf - 7) // 2 * 2
    tc.host_program.assert_same((part.vertices, part.faces[:whole], part.rgb, part.normals) + _as_tuple(part)[4:],
                                (full.vertices[:nv - 11], full.faces[:whole], full.rgb[:nv - 11], full.normals[:nv - 11]) + _as_tuple(full)[4:],
                                KEYS, "capacities below the totals")
    with pytest.raises(ValueError, match="tsdf_mesh: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least"):
        tsdfmesh.tsdf_mesh(vol, workspace=work[:need - 1])
    with pytest.raises(ValueError, match="tsdf_mesh: workspace must be"):
        tsdfmesh.tsdf_mesh(vol, workspace=work[1:])


# ---- guarded C-ABI ------------------------------------------------------------------------------------------------------------------

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


def test_guarded_mesh():
    """ud_tsdf_mesh on guarded allocations: fp32 outputs off 16-byte boundaries, u8 colours at an odd offset, a dirty workspace; capacities
    at, below (an odd number of triangles: the last row keeps its guard bits, no half quad) and at zero; absent outputs untouched"""
    from unidepth_amd import _lib, tsdfmesh
    from unidepth_amd.ops import check, cur_stream, mk
    s = _field((5, 19, 23), 7, B=3)
    s["weight"] = s["weight"].copy()
    s["weight"][1] = 0
    vol = _volume(s)
    want = tsdfmesh.tsdf_mesh(vol, rgb_dtype=torch.float32, return_normals=True)
    want8 = tsdfmesh.tsdf_mesh(vol)
    nv, nf = want.vertices.shape[0], want.faces.shape[0]
    assert nv > 1024 and nf > 1024 and int(want.vert_counts[1]) == 0
    need = int(_lib.lib.ud_tsdf_mesh_work_bytes(3, 23, 19, 5))
    for f32, with_rgb, with_normals, with_faces, vcap, fcap in ((0, True, True, True, nv, nf), (1, True, False, True, nv - 5, nf - 9),
                                                                (0, False, True, False, nv, nf), (0, True, True, True, 0, 0),
                                                                (1, False, False, True, 0, nf), (0, True, True, True, nv, 1)):
        bufs = dict(vertices=_Out(3 * max(vcap, 1), torch.float32, 1), rgb=_Out(3 * max(vcap, 1), torch.float32 if f32 else torch.uint8, 3),
                    normals=_Out(3 * max(vcap, 1), torch.float32, 3), faces=_Out(3 * max(fcap, 1), torch.int32, 1),
                    vert_counts=_Out(3, torch.int64, 1), vert_offsets=_Out(4, torch.int64, 1), face_counts=_Out(3, torch.int64, 1),
                    face_offsets=_Out(4, torch.int64, 1))
        work = torch.full((need + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        ptr = lambda k, on: bufs[k].t.data_ptr() if on else None  # noqa: E731
        desc = mk(_lib.UdTsdfMesh, tsdf=vol.tsdf, weight=vol.weight, color=vol.color, origin=vol.origin, vertices=ptr("vertices", vcap),
                  rgb=ptr("rgb", with_rgb and vcap), normals=ptr("normals", with_normals and vcap), faces=ptr("faces", with_faces and fcap),
                  vert_counts=ptr("vert_counts", True), vert_offsets=ptr("vert_offsets", True), face_counts=ptr("face_counts", True),
                  face_offsets=ptr("face_offsets", True), work=work, work_bytes=need, vert_capacity=vcap, face_capacity=fcap, B=3, Nx=23, Ny=19,
                  Nz=5, n_origin=3, rgb_f32=f32, voxel_size_bits=tc.f32_bits(vol.voxel_size), min_weight_bits=tc.f32_bits(1.0))
        check(_lib.lib.ud_tsdf_mesh(desc, cur_stream()), "ud_tsdf_mesh")
        torch.cuda.synchronize()
        assert bool((work[need:] == 0xFF).all())
        for k in KEYS[4:]:
            assert torch.equal(bufs[k].t, getattr(want, k)), k
            bufs[k].check(k)
        whole = fcap // 2 * 2 if fcap < nf else nf                                 # the triangles of complete quads below the capacity
        bufs["vertices"].check("vertices", written=vcap > 0, upto=3 * min(vcap, nv))
        bufs["rgb"].check("rgb", written=bool(with_rgb and vcap), upto=3 * min(vcap, nv))
        bufs["normals"].check("normals", written=bool(with_normals and vcap), upto=3 * min(vcap, nv))
        bufs["faces"].check("faces", written=bool(with_faces and fcap), upto=3 * whole)
        if vcap:
            assert torch.equal(tc.bits(bufs["vertices"].t.view(-1, 3)[:vcap]), tc.bits(want.vertices[:vcap]))
            if with_rgb:
                assert torch.equal(tc.bits(bufs["rgb"].t.view(-1, 3)[:vcap]), tc.bits((want if f32 else want8).rgb[:vcap]))
            if with_normals:
                assert torch.equal(tc.bits(bufs["normals"].t.view(-1, 3)[:vcap]), tc.bits(want.normals[:vcap]))
        if with_faces and whole:
            assert torch.equal(bufs["faces"].t.view(-1, 3)[:whole], want.faces[:whole])


# ---- the composition and the graph --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("special", "field"))
def test_composition_on_the_gpu_equals_the_kernel(name):
    from unidepth_amd import tsdfmesh
    s = mc.batch(("special", "hole", "pair"), per_origin=True) if name == "special" else _field((9, 35, 40), 11, B=2)
    vol = _volume(s)
    for dtype in (torch.uint8, torch.float32):
        got = tsdfmesh.tsdf_mesh(vol, rgb_dtype=dtype, return_normals=True)
        want = tsdfmesh.tsdf_mesh_composition(vol, rgb_dtype=dtype, return_normals=True)
        assert want.vertices.is_cuda and want.vertices.shape[0] > 300
        tc.host_program.assert_same(_as_tuple(got), _as_tuple(want), KEYS, f"{name} {dtype}")


def test_graph_replay_after_the_volume_was_rewritten():
    """captured once with both capacities; replayed after the volume's distances, weights and colours were rewritten in place: each replay
    equals the eager call and the restatement"""
    from unidepth_amd import tsdfmesh
    a, b = mc.batch(("sphere", "hole"), per_origin=True), mc.batch(("pair", "special"), per_origin=True)
    vol = _volume(a)
    vcap, fcap = 500, 900

    def fn():
        return tsdfmesh.tsdf_mesh(vol, vert_capacity=vcap, face_capacity=fcap, return_normals=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sm = fn()
    for k in range(3):
        s = b if k % 2 == 0 else a
        vol.tsdf.copy_(_dev(s["tsdf"]))
        vol.weight.copy_(_dev(s["weight"]))
        vol.color.copy_(_dev(s["color"]))
        graph.replay()
        torch.cuda.synchronize()
        p = mc.packed(mc.cells(s["tsdf"], s["weight"], s["color"], s["origin"], s["voxel"], 1.0))
        nv, nf = len(p["vertices"]), len(p["faces"])
        assert 0 < nv <= vcap and 0 < nf <= fcap
        got = (sm.vertices[:nv], sm.faces[:nf], sm.rgb[:nv], sm.normals[:nv]) + _as_tuple(sm)[4:]
        tc.host_program.assert_same(got, _want(p), KEYS, f"replay {k}")
