"""tsdf_mesh without a GPU (unidepth_amd/tsdfmesh.py, include/unidepth_hip.h UdTsdfMesh): csrc/tsdf_mesh_point.h compiled for the host into
tests/tsdf_mesh_host (stand-alone, under AddressSanitizer and UBSan) against the numpy fp32 restatement of tests/tsdf_mesh_common.py, bit
for bit; the topology of the meshes on the restatement and on the header alike; the known answers; the torch composition on CPU tensors
against the restatement; the C-ABI refusals, the Python argument errors and the PLY writer.

Figures the issue's prototype gave that this file reproduces: the sphere has 180 vertices, 356 edges, 178 quads and 178 live slots,
18.75 % of its cells live, windings 29/29, 30/30, 30/30.  The prototype's pair of spheres (132 / 256 / 128) and its draw of zeroed weights
(89 / 66 / 30 of 153) had parameters the issue does not state: the pair here has 140 / 272 / 136 and the draw 98 / 78 / 41 of 153, under
the same assertions."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import tsdf_common as tc
import tsdf_mesh_common as mc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return mc.build_host(tmp_path_factory)


@pytest.fixture(scope="module")
def hosted(exe):
    """name -> the host program's result on the scene, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            s = mc.scene(name)
            cache[name] = mc.host_cells(exe, s["tsdf"], s["weight"], s["color"], s["origin"], s["voxel"], s["min_weight"])
        return cache[name]
    return get


# ---- the header against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.SCENES)
def test_header_matches_the_restatement(hosted, name):
    got, want = hosted(name), mc.restated(name)
    mc.assert_same_cells(got, want, name)
    assert mc.same_bits(got["rgb_u8"], np.where(want["live"][..., None], tc.to_u8(want["rgb"]), 0).astype(np.uint8))
    mc.assert_not_vacuous(name, mc.scene(name), want)
    # every quad belongs to a live slot, and the slots are tsdf_points' own
    s = mc.scene(name)
    assert not (want["quad_live"] & ~want["slot_live"]).any()
    assert np.array_equal(want["slot_live"], tc.slots(s["tsdf"], s["weight"], None, s["origin"], s["voxel"], s["min_weight"])[0])


def test_header_on_a_batch_without_colour_and_with_origins(exe):
    s = mc.batch(("sphere", "hole", "special"), per_origin=True)
    for color, mw in ((None, 1.0), (s["color"], 0.5)):
        got = mc.host_cells(exe, s["tsdf"], s["weight"], color, s["origin"], s["voxel"], mw)
        want = mc.cells(s["tsdf"], s["weight"], color, s["origin"], s["voxel"], mw)
        mc.assert_same_cells(got, want, f"batch colour={color is not None}")
        assert want["live"].sum(axis=1).tolist() == [mc.restated(n)["live"].sum() for n in ("sphere", "hole", "special")]


def test_special_values_are_in_the_scene():
    t = mc.scene("special")["tsdf"]
    r = mc.restated("special")
    assert np.isnan(t).any() and np.isposinf(t).any() and np.isneginf(t).any() and (t == 0).any() and (np.signbit(t) & (t == 0)).any()
    B, Nz, Ny, Nx = t.shape
    n = Nz * Ny * Nx
    flat, live = t.reshape(-1), r["slot_live"].reshape(n, 3)
    step = (1, Nx, Nx * Ny)
    zero_low = zero_high = False
    for axis in range(3):
        s = np.nonzero(live[:, axis])[0]
        zero_low |= bool((flat[s] == 0).any())
        zero_high |= bool((flat[s + step[axis]] == 0).any())
    assert zero_low and zero_high                      # an exact zero at either end of a live edge: t = 0 / (0 - b) and a / (a - 0)
    # a NaN corner kills the cell
    iz, iy, ix = np.argwhere(np.isnan(t[0]))[0]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                z, y, x = iz - dz, iy - dy, ix - dx
                if min(z, y, x) >= 0:
                    assert not r["live"][0, (z * Ny + y) * Nx + x]


# ---- topology -----------------------------------------------------------------------------------------------------------------------

def _check_closed(name, r, spheres, want_euler):
    p = mc.packed(r)
    top = mc.topology(p["quads"], len(p["vertices"]))
    assert top["closed"] and top["oriented"], (name, top)
    assert top["euler"] == want_euler, (name, top)
    assert top["F"] == int(r["slot_live"].sum()), (name, top)                   # one quad per point of tsdf_points
    assert len(top["referenced"]) == top["V"], (name, top)
    v, f, nrm = p["vertices"].astype(np.float64), p["faces"], p["normals"].astype(np.float64)
    centres = np.array([c for c, _ in spheres])
    tri = v[f]
    geo = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    centroid = tri.mean(axis=1)
    nearest = centres[np.argmin(((centroid[:, None] - centres[None]) ** 2).sum(-1), axis=1)]
    assert ((geo * (centroid - nearest)).sum(-1) > 0).all(), name
    nearest_v = centres[np.argmin(((v[:, None] - centres[None]) ** 2).sum(-1), axis=1)]
    assert ((nrm * (v - nearest_v)).sum(-1) > 0).all(), name
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-6)
    return top


def test_sphere_topology(hosted):
    for r in (mc.restated("sphere"), dict(hosted("sphere"), slot_live=mc.restated("sphere")["slot_live"])):
        top = _check_closed("sphere", r, ((mc.CENTRE, mc.RADIUS),), 2)
        assert (top["V"], top["E"], top["F"]) == (180, 356, 178) and int(r["slot_live"].sum()) == 178
    r = mc.restated("sphere")
    assert mc.live_share(mc.scene("sphere"), r) == 0.1875
    assert mc.windings(r) == [(29, 29), (30, 30), (30, 30)]
    # the vertices lie on the sphere to within the discretisation: a fifth of a voxel
    v = mc.packed(r)["vertices"].astype(np.float64)
    assert np.abs(np.linalg.norm(v - np.array(mc.CENTRE), axis=1) - mc.RADIUS).max() < 0.2 * mc.VOXEL


def test_two_spheres_topology(hosted):
    for r in (mc.restated("pair"), dict(hosted("pair"), slot_live=mc.restated("pair")["slot_live"])):
        top = _check_closed("pair", r, mc.PAIR, 4)
        assert (top["V"], top["E"], top["F"]) == (140, 272, 136)


def test_weights_hole_leaves_unreferenced_vertices_and_slots_without_quads(hosted):
    for r in (mc.restated("hole"), hosted("hole")):
        p = mc.packed(r)
        top = mc.topology(p["quads"], len(p["vertices"]))
        slots = int(mc.restated("hole")["slot_live"].sum())
        assert (top["V"], len(top["referenced"]), top["F"], slots) == (98, 78, 41, 153)
        assert len(top["referenced"]) < top["V"] and top["F"] < slots
        assert top["wound"] and not top["closed"]                                  # open, but still consistently wound


# ---- known answers ------------------------------------------------------------------------------------------------------------------

def _run_both(exe, t, w, voxel=0.25, origin=((0.0, 0.0, 0.0),)):
    o = np.array(origin, np.float32)
    got = mc.host_cells(exe, t, w, None, o, voxel, 1.0)
    want = mc.cells(t, w, None, o, voxel, 1.0)
    mc.assert_same_cells(got, want)
    return mc.packed(got)


def test_plane_known_answer(exe):
    for below_positive, first in ((True, [0, 6, 7, 1]), (False, [0, 1, 7, 6])):
        p = _run_both(exe, *mc.plane((3, 5, 7), below_positive))
        assert len(p["vertices"]) == 24 and len(p["quads"]) == 15 and len(p["faces"]) == 30
        assert p["quads"][0].tolist() == first
        assert p["faces"][:2].tolist() == [[first[0], first[1], first[2]], [first[0], first[2], first[3]]]
        assert p["vert_counts"].tolist() == [24] and p["face_counts"].tolist() == [30] and p["face_offsets"].tolist() == [0, 30]
        nz = -1.0 if below_positive else 1.0
        assert np.array_equal(p["normals"], np.broadcast_to(np.array([0, 0, nz], np.float32), (24, 3)))
        tri = p["vertices"][p["faces"]].astype(np.float64)
        assert (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])[:, 2] * nz > 0).all()
    p = _run_both(exe, *mc.plane((3, 3, 3), True))
    assert len(p["vertices"]) == 4 and p["quads"].tolist() == [[0, 2, 3, 1]]
    p = _run_both(exe, *mc.plane((2, 2, 2), True))
    assert len(p["vertices"]) == 1 and len(p["quads"]) == 0 and p["faces"].shape == (0, 3)
    # -0.0 counts as not negative: alone among positive corners it leaves the cell all of one sign, alone among negative ones it makes it live
    for others, n_vertices in ((1.0, 0), (-1.0, 1)):
        t = np.full((1, 2, 2, 2), others, np.float32)
        t[0, 1, 0, 1] = -0.0
        assert len(_run_both(exe, t, np.ones_like(t))["vertices"]) == n_vertices
    for grid in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        t = np.random.RandomState(1).normal(size=(1,) + grid).astype(np.float32)
        p = _run_both(exe, t, np.ones_like(t))
        assert len(p["vertices"]) == 0 and len(p["faces"]) == 0 and p["vert_offsets"].tolist() == [0, 0]


def test_vertex_height_is_within_four_ulp_of_the_crossing(exe):
    """the four z edges of a cell of a tilted-free plane cross at one height h; the vertex is ((h + h) + h + h) / 4: three additions and
    a division, each within half an ulp of a value within a factor of four of h, so at most 4 ulp of h"""
    t, w = mc.plane((3, 5, 7), True)
    t = np.where(t > 0, np.float32(0.3), np.float32(-0.7)).astype(np.float32)
    p = _run_both(exe, t, w, voxel=0.1, origin=((0.013, -0.4, 0.77),))
    a, b = np.float32(0.3), np.float32(-0.7)
    h = (np.float32(0.77) + (np.float32(0) + np.float32(0.5)) * np.float32(0.1)) + (a / (a - b)) * np.float32(0.1)      # tsdf_points' crossing
    assert abs(float(h) - (0.77 + 0.05 + 0.03)) < 1e-6
    ulp = float(np.spacing(np.float32(h)))
    assert (np.abs(p["vertices"][:, 2].astype(np.float64) - float(h)) <= 4 * ulp).all()


# ---- the torch composition on CPU tensors -------------------------------------------------------------------------------------------

def _volume(s, color=True, device="cpu"):
    from unidepth_amd import tsdf
    f = lambda a: torch.from_numpy(np.array(a, np.float32)).to(device)  # noqa: E731
    return tsdf.TsdfVolume(f(s["tsdf"]), f(s["weight"]), f(s["color"]) if color else None, f(s["origin"]), s["voxel"])


def assert_mesh_equals(m, p, what=""):
    """a TriangleMesh against packed()'s dict, bit for bit"""
    for k in ("vertices", "faces", "rgb", "normals", "vert_counts", "vert_offsets", "face_counts", "face_offsets"):
        a, b = getattr(m, k), p[k]
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and mc.same_bits(a, b), (what, k, a.shape, b.shape)


@pytest.mark.parametrize("name", mc.SCENES)
def test_composition_on_cpu_matches_the_restatement(name):
    from unidepth_amd import tsdfmesh
    s, r = mc.scene(name), mc.restated(name)
    for dtype in (torch.uint8, torch.float32):
        m = tsdfmesh.tsdf_mesh_composition(_volume(s), rgb_dtype=dtype, return_normals=True)
        assert_mesh_equals(m, mc.packed(r, rgb_u8=dtype == torch.uint8), name)
    m = tsdfmesh.tsdf_mesh_composition(_volume(s, color=False))
    assert m.rgb is None and m.normals is None
    assert_mesh_equals(m, dict(mc.packed(r), rgb=None, normals=None), name)


def test_composition_on_a_batch_and_on_grids_without_cells():
    from unidepth_amd import tsdfmesh
    s = mc.batch(("sphere", "hole", "pair"), per_origin=True)
    s["weight"] = s["weight"].copy()
    s["weight"][1] = 0                                                            # an empty middle member
    r = mc.cells(s["tsdf"], s["weight"], s["color"], s["origin"], s["voxel"], 1.0)
    m = tsdfmesh.tsdf_mesh_composition(_volume(s), return_normals=True)
    assert_mesh_equals(m, mc.packed(r), "batch")
    assert m.vert_counts.tolist() == [180, 0, 140] and m.face_counts.tolist() == [356, 0, 272]
    parts = m.split()
    assert [len(x.vertices) for x in parts] == [180, 0, 140] and int(parts[2].faces.max()) == 139 and parts[2].face_offsets.tolist() == [0, 272]
    for grid in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        t = np.random.RandomState(2).normal(size=(2,) + grid).astype(np.float32)
        e = dict(tsdf=t, weight=np.ones_like(t), color=np.zeros((2, 3) + grid, np.float32), origin=np.zeros((1, 3), np.float32), voxel=0.5)
        m = tsdfmesh.tsdf_mesh_composition(_volume(e), return_normals=True)
        assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.faces.dtype == torch.int32 and m.rgb.dtype == torch.uint8
        assert m.vert_offsets.tolist() == [0, 0, 0] and m.face_counts.tolist() == [0, 0] and m.normals.shape == (0, 3)


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------------

def test_tsdf_mesh_workspace_size():
    """cp_layout(B, n) then cp_layout(B, 3n), 136 bytes per tile of 1024 items"""
    from unidepth_amd import _lib
    wb, pb = _lib.lib.ud_tsdf_mesh_work_bytes, _lib.lib.ud_tsdf_points_work_bytes
    assert wb(1, 341, 1, 1) == 136 + 136 and wb(1, 342, 1, 1) == 136 + 272 and wb(3, 683, 3, 1) == 3 * (3 + 7) * 136
    assert wb(2, 40, 50, 60) == pb(2, 40, 50, 60) + 2 * 118 * 136 and wb(2, 40, 50, 60) % 8 == 0
    assert wb(0, 1, 1, 1) == -1 and wb(1, 0, 1, 1) == -1 and wb(1, 1024, 1024, 683) == -1 and wb(65536, 1, 1, 1) == -1


def test_every_refusal_of_mesh():
    """every refusal comes back before any HIP call: this runs without a GPU, on made-up addresses"""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_tsdf_mesh(None, None) == -1 and "null descriptor" in lib.ud_last_error().decode()
    need = lib.ud_tsdf_mesh_work_bytes(2, 4, 5, 6)

    def call(**kw):
        d = _lib.UdTsdfMesh()
        base = dict(tsdf=16, weight=16, color=None, origin=16, vertices=16, rgb=None, normals=None, faces=16, vert_counts=16, vert_offsets=16,
                    face_counts=16, face_offsets=16, work=16, work_bytes=need, vert_capacity=10, face_capacity=10, B=2, Nx=4, Ny=5, Nz=6,
                    n_origin=1, rgb_f32=0, voxel_size_bits=tc.f32_bits(0.1), min_weight_bits=tc.f32_bits(1.0))
        base.update(kw)
        for k, v in base.items():
            setattr(d, k, v)
        return lib.ud_tsdf_mesh(C.byref(d), None), lib.ud_last_error().decode()
    for kw, msg in (
            (dict(B=0), "bad sizes"), (dict(B=65536), "bad sizes"), (dict(Nx=0), "bad sizes"), (dict(Ny=-1), "bad sizes"), (dict(Nz=0), "bad sizes"),
            (dict(vert_capacity=-1), "bad sizes"), (dict(face_capacity=-1), "bad sizes"), (dict(Nx=1 << 10, Ny=1 << 10, Nz=683), "bad sizes"),
            (dict(Nx=2 ** 31 - 1, Ny=2 ** 31 - 1, Nz=2), "bad sizes"),
            (dict(tsdf=None), "null pointer"), (dict(weight=None), "null pointer"), (dict(origin=None), "null pointer"),
            (dict(vert_counts=None), "null pointer"), (dict(vert_offsets=None), "null pointer"), (dict(face_counts=None), "null pointer"),
            (dict(face_offsets=None), "null pointer"), (dict(work=None), "null pointer"), (dict(work=20), "null pointer"),
            (dict(rgb=16), "rgb needs"), (dict(rgb=16, color=16, vertices=None), "rgb needs"), (dict(normals=16, vertices=None), "normals need"),
            (dict(n_origin=0), "n_origin"), (dict(n_origin=3), "n_origin"),
            (dict(voxel_size_bits=tc.f32_bits(float("nan"))), "voxel_size"), (dict(voxel_size_bits=tc.f32_bits(float("inf"))), "voxel_size"),
            (dict(voxel_size_bits=tc.f32_bits(0.0)), "voxel_size"), (dict(voxel_size_bits=tc.f32_bits(-1.0)), "voxel_size"),
            (dict(min_weight_bits=tc.f32_bits(float("nan"))), "min_weight"),
            (dict(work_bytes=need - 1), "workspace smaller"), (dict(work_bytes=0), "workspace smaller")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err and err.startswith("ud_tsdf_mesh: "), (kw, rc, err)


# ---- argument checks, no GPU ------------------------------------------------------------------------------------------------------

def test_argument_errors_without_gpu():
    import unidepth_amd
    from unidepth_amd import tsdf, tsdfmesh
    vol = _volume(mc.scene("sphere"))
    for f in (tsdfmesh.tsdf_mesh, tsdfmesh.tsdf_mesh_composition, vol.mesh):
        fn = "tsdf_mesh" if f == vol.mesh else f.__name__
        call = (lambda **kw: f(**kw)) if f == vol.mesh else (lambda **kw: f(vol, **kw))
        for mw, msg in (("x", "must be a number in fp32's range"), (None, "must be a number in fp32's range"), (1e300, "must be a number in fp32's range"),
                        (float("nan"), "must be a number, got"), (True, "must be a number, got")):
            with pytest.raises(ValueError, match=f"{fn}: min_weight {msg}"):
                call(min_weight=mw)
        for dt in (torch.float16, torch.int32, None, "uint8"):
            with pytest.raises(ValueError, match=f"{fn}: rgb_dtype must be torch.uint8 or torch.float32"):
                call(rgb_dtype=dt)
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="tsdf_mesh: vert_capacity must be a non-negative int or None"):
            tsdfmesh.tsdf_mesh(vol, vert_capacity=bad, face_capacity=4)
        with pytest.raises(ValueError, match="tsdf_mesh: face_capacity must be a non-negative int or None"):
            tsdfmesh.tsdf_mesh(vol, vert_capacity=4, face_capacity=bad)
    for kw in (dict(vert_capacity=10), dict(face_capacity=10)):
        with pytest.raises(ValueError, match="tsdf_mesh: vert_capacity and face_capacity go together"):
            tsdfmesh.tsdf_mesh(vol, **kw)
    # the volume, in tsdf_points' sentences; well-formed arguments on the CPU: the HIP kernels are the only implementation of tsdf_mesh
    with pytest.raises(ValueError, match="tsdf_mesh: volume.tsdf must be a contiguous fp32 GPU tensor"):
        tsdfmesh.tsdf_mesh(vol)
    with pytest.raises(ValueError, match="tsdf_mesh: volume.tsdf must be a contiguous fp32 GPU tensor"):
        vol.mesh(vert_capacity=10, face_capacity=10, return_normals=True)
    for f in (tsdfmesh.tsdf_mesh, tsdfmesh.tsdf_mesh_composition):
        with pytest.raises(ValueError, match=f"{f.__name__}: volume must be a TsdfVolume, got Tensor"):
            f(vol.tsdf)
    c = tsdfmesh.tsdf_mesh_composition
    V = tsdf.TsdfVolume
    for v, msg in ((V(vol.tsdf[0], vol.weight, None, vol.origin, 0.1), "volume.tsdf"), (V(vol.tsdf.double(), vol.weight, None, vol.origin, 0.1), "volume.tsdf"),
                   (V(vol.tsdf, vol.weight[:, 1:], None, vol.origin, 0.1), "volume.weight"), (V(vol.tsdf, vol.weight, vol.color[:, :2], vol.origin, 0.1), "volume.color"),
                   (V(vol.tsdf, vol.weight, None, torch.zeros(3), 0.1), "volume.origin"), (V(vol.tsdf, vol.weight, None, torch.zeros(2, 3), 0.1), "volume.origin"),
                   (V(vol.tsdf, vol.weight, None, vol.origin, 0.0), "volume.voxel_size"), (V(vol.tsdf, vol.weight, None, vol.origin, "a"), "volume.voxel_size"),
                   (V(vol.tsdf, vol.weight, None, vol.origin, float("inf")), "volume.voxel_size")):
        with pytest.raises(ValueError, match=f"tsdf_mesh_composition: {msg}"):
            c(v)
    huge = torch.zeros(1).expand(1, 683, 1024, 1024)                               # no memory behind it: 3 * n is beyond the slots' limit
    with pytest.raises(ValueError, match="tsdf_mesh_composition: unsupported sizes B=1 grid=683x1024x1024"):
        c(V(huge, huge, None, vol.origin, 0.1))
    for name in ("TriangleMesh", "tsdf_mesh", "tsdf_mesh_composition", "save_mesh_ply"):
        assert name in unidepth_amd.__all__ and getattr(unidepth_amd, name) is getattr(tsdfmesh, name)
    assert "NO host synchronisation" in tsdfmesh.tsdf_mesh.__doc__ and "unreferenced vertex" in tsdfmesh.tsdf_mesh.__doc__


# ---- the PLY writer ---------------------------------------------------------------------------------------------------------------

def _parse_ply(data):
    """a parser of its own: the header line by line, then the vertex rows and the face list by the declared properties"""
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == ""
    elements = []
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        else:
            assert w[0] == "property"
            elements[-1][2].append(tuple(w[1:]))
    assert [e[0] for e in elements] == ["vertex", "face"]
    (_, nv, vprops), (_, nf, fprops) = elements
    assert fprops == [("list", "uchar", "int", "vertex_indices")]
    fmt = {"float": "f", "uchar": "B"}
    row = struct.Struct("<" + "".join(fmt[p[0]] for p in vprops))
    verts = [row.unpack_from(body, k * row.size) for k in range(nv)]
    at = nv * row.size
    faces = []
    for _ in range(nf):
        assert body[at] == 3
        faces.append(struct.unpack_from("<3i", body, at + 1))
        at += 13
    assert at == len(body)
    return [p[1] for p in vprops], verts, faces


def test_save_mesh_ply_round_trip(tmp_path):
    from unidepth_amd import tsdfmesh
    m = tsdfmesh.tsdf_mesh_composition(_volume(mc.scene("sphere")), return_normals=True)
    path = str(tmp_path / "sphere.ply")
    tsdfmesh.save_mesh_ply(path, m.vertices, m.faces, m.rgb, m.normals)
    names, verts, faces = _parse_ply(open(path, "rb").read())
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    v, nrm, rgb, f = m.vertices.numpy(), m.normals.numpy(), m.rgb.numpy(), m.faces.numpy()
    assert len(verts) == 180 and len(faces) == 356
    got = np.array([r[:6] for r in verts], np.float32)
    assert mc.same_bits(got, np.concatenate([v, nrm], axis=1)) and np.array_equal(np.array([r[6:] for r in verts], np.uint8), rgb)
    assert np.array_equal(np.array(faces, np.int32), f)
    # byte for byte: the header, the rows, the list
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex 180\n" + "".join(f"property float {n}\n" for n in names[:6])
            + "".join(f"property uchar {n}\n" for n in names[6:]) + "element face 356\nproperty list uchar int vertex_indices\nend_header\n").encode()
    rows = b"".join(v[k].tobytes() + nrm[k].tobytes() + rgb[k].tobytes() for k in range(180))
    tris = b"".join(b"\x03" + f[k].astype("<i4").tobytes() for k in range(356))
    assert open(path, "rb").read() == want + rows + tris
    # plain: vertices and faces only, arrays; and the refusals
    tsdfmesh.save_mesh_ply(path, v, f)
    names, verts, faces = _parse_ply(open(path, "rb").read())
    assert names == ["x", "y", "z"] and len(verts) == 180 and np.array_equal(np.array(faces, np.int32), f)
    for args, msg in (((v[:, :2], f), "vertices must be"), ((v, f[:, :2]), "faces must be"), ((v, f.astype(np.float32)), "faces must be"),
                      ((v[:10], f), "faces index outside"), ((v, f, rgb[:5]), "rgb must be"), ((v, f, None, nrm[:5]), "normals must be")):
        with pytest.raises(ValueError, match=f"save_mesh_ply: {msg}"):
            tsdfmesh.save_mesh_ply(path, *args)
