"""Point-cloud packing without a GPU (unidepth_amd/pointcloud.py, include/unidepth_hip.h UdPointCloud): the numpy restatement of
tools/make_golden_pointcloud.py against the reference's own arrays (tests/golden/pointcloud.npz), the C-ABI's argument
checks and workspace query, the PLY writers, and pack_points' argument errors."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_pointcloud", os.path.join(ROOT, "tools", "make_golden_pointcloud.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

TILE = 1024          # csrc/compact.h CP_TILE


def test_golden_has_every_case():
    g = np.load(mg.GOLDEN)
    assert sorted(g.files) == sorted(mg.CASES)
    for name, (H, W, frac) in mg.CASES.items():
        a = g[name]
        assert a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 6
        assert a.shape[0] == int(mg.case_inputs(name)[2].sum())
        assert abs(a.shape[0] / (H * W) - frac) < 0.05
    assert os.path.getsize(mg.GOLDEN) < 64 * 1024


@pytest.mark.parametrize("name", list(mg.CASES))
def test_restatement_matches_reference_golden(name):
    """row count, order, z and colours exact; x / y exact too, the restatement computing them in float64 as the reference does"""
    image, depth, mask, K = mg.case_inputs(name)
    got = mg.restate_rgbd(image, depth, mask, K)
    ref = np.load(mg.GOLDEN)[name]
    assert got.dtype == np.float64 and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)
    ys, xs = np.nonzero(mask)                                   # numpy boolean-index order
    np.testing.assert_array_equal(ref[:, 2], depth[ys, xs].astype(np.float64))
    np.testing.assert_array_equal(ref[:, 3:], image[ys, xs].astype(np.float64))
    assert (ref[:, 1] * (ys - K[1, 2]) <= 0).all()              # +y up


def test_restatement_predicate_cases():
    """the restated predicate on hand-made maps: NaN / inf, thresholds met exactly, an edge step exactly on edge_rtol"""
    d = np.array([[[1.0, 1.25, 1.25, 2.0], [1.0, np.nan, 1.25, np.inf]]], dtype=np.float32)
    assert mg.valid_mask(depth=d).tolist() == [[[True, True, True, True], [True, False, True, False]]]
    assert mg.valid_mask(depth=d, depth_range=(1.25, 2.0)).tolist() == [[[False, True, True, True], [False, False, True, False]]]
    # 1 -> 1.25: |step| = 0.25 = 0.25 * min: kept at rtol 0.25; 1.25 -> 2: dropped; NaN / inf neighbours drop their neighbours
    assert mg.valid_mask(depth=d, edge_rtol=0.25).tolist() == [[[True, False, False, False], [False, False, False, False]]]
    c = np.array([[[0.5, np.nan, 0.49999997, 1.0], [0.5, 0.5, 0.5, 0.5]]], dtype=np.float32)
    assert mg.valid_mask(depth=d, confidence=c, min_confidence=0.5).tolist() == [[[True, False, False, True], [True, False, True, False]]]
    p = np.zeros((1, 3, 2, 4), dtype=np.float32)
    p[0, 0, 0, 1] = np.inf
    p[0, 1, 1, 2] = np.nan
    r = mg.restate(points=p, mask=np.ones((1, 2, 4), dtype=bool))
    assert r["index"].tolist() == [0, 2, 3, 4, 5, 7] and r["counts"].tolist() == [6] and r["offsets"].tolist() == [0, 6]


@pytest.mark.skipif(not os.path.isfile(mg.reference_path()), reason="reference tree not present (authoring machine only)")
def test_reference_rerun_reproduces_golden():
    ref = mg.reference_get_pointcloud_from_rgbd()
    g = np.load(mg.GOLDEN)
    for name in mg.CASES:
        np.testing.assert_array_equal(mg.reference_output(ref, name), g[name], err_msg=name)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------

def test_pack_rejects_bad_descriptors_without_a_launch():
    """every refusal comes back before any HIP call: this runs on a machine without a GPU, the pointers are never followed"""
    from unidepth_amd import _lib
    lib = _lib.lib
    P = 0x1000                                      # stands for a device pointer
    B, H, W = 2, 5, 7
    nbytes = lib.ud_pointcloud_work_bytes(B, H, W)

    def rc(**kw):
        base = dict(points=P, counts=P, offsets=P, work=P, work_bytes=nbytes, capacity=10, xyz=P, B=B, H=H, W=W)
        base.update(kw)
        d = _lib.UdPointCloud()
        for k, v in base.items():
            setattr(d, k, v)
        r = lib.ud_pointcloud_pack(C.byref(d), None)
        return r, lib.ud_last_error().decode()

    r, msg = lib.ud_pointcloud_pack(None, None), lib.ud_last_error().decode()
    assert r < 0 and "null descriptor" in msg
    for kw, word in ((dict(points=None), "neither points nor depth"),
                     (dict(points=None, depth=P), "depth mode needs K"),
                     (dict(points=None, depth=P, K=P, nK=3), "nK"),
                     (dict(points=None, depth=P, K=P, nK=0), "nK"),
                     (dict(work_bytes=nbytes - 1), "workspace smaller"),
                     (dict(work=None), "null pointer"),
                     (dict(counts=None), "null pointer"),
                     (dict(offsets=None), "null pointer"),
                     (dict(flags=_lib.UD_PC_MINCONF), "UD_PC_MINCONF without a confidence"),
                     (dict(flags=16), "unknown flag"),
                     (dict(B=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=-1), "bad sizes"), (dict(B=65536), "bad sizes"),
                     (dict(H=65536, W=65536), "bad sizes"),
                     (dict(capacity=-1), "bad sizes"),
                     (dict(B=3, H=32768, W=32768, index=P, work_bytes=1 << 40), "B*H*W"),
                     (dict(image=P, image_f32=P, rgb=P), "one colour input"),
                     (dict(image=P), "one colour input")):
        r, msg = rc(**kw)
        assert r < 0 and word in msg, (kw, r, msg)


def test_work_bytes_monotone_and_covers_bitmask_and_tile_counts():
    from unidepth_amd import _lib
    wb = _lib.lib.ud_pointcloud_work_bytes
    for B, H, W in ((1, 1, 1), (1, 32, 32), (3, 37, 53), (8, 518, 518), (8, 480, 640)):
        n = wb(B, H, W)
        tiles = B * -(-H * W // TILE)
        assert n >= tiles * TILE // 8 + tiles * 4                # one bit per pixel of every tile + an int32 count per tile
        assert n <= tiles * TILE // 8 + tiles * 8 + 256
        assert wb(B + 1, H, W) >= n and wb(B, H + 1, W) >= n and wb(B, H, W + 1) >= n
        assert wb(B + 1, H, W) > n and wb(B, H + TILE, W) > n and wb(B, H, W + TILE) > n
    assert wb(0, 4, 4) < 0 and wb(1, 0, 4) < 0 and wb(1, 4, -1) < 0 and wb(1, 65536, 65536) < 0


# ---- PLY writers ---------------------------------------------------------------------------------------------------------------------

def _read_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[-1] == "end_header"
    n = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    return lines, n, props, end


@pytest.mark.parametrize("n,colour", [(57, True), (57, False), (0, True), (0, False)])
def test_save_ply_binary_roundtrip(tmp_path, n, colour):
    from unidepth_amd import save_ply
    rng = np.random.default_rng(n + colour)
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    if n:
        xyz[0] = [np.float32(1e-42), -0.0, 3.4e38]                 # a subnormal, a signed zero, a large value: bits, not values
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8) if colour else None
    path = tmp_path / "cloud.ply"
    save_ply(str(path), torch.from_numpy(xyz), rgb)
    lines, count, props, off = _read_ply(path)
    assert lines[1] == "format binary_little_endian 1.0" and count == n
    want = [["float", "x"], ["float", "y"], ["float", "z"]] + ([["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]] if colour else [])
    assert props == want
    dt = np.dtype([(name, "<f4" if t == "float" else "u1") for t, name in props])
    assert os.path.getsize(path) == off + n * dt.itemsize
    rows = np.fromfile(path, dtype=dt, offset=off)
    assert rows.shape == (n,)
    got = np.stack([rows[k] for k in "xyz"], axis=-1) if n else np.zeros((0, 3), np.float32)
    assert np.array_equal(got.view(np.uint32), xyz.view(np.uint32))
    if colour and n:
        assert np.array_equal(np.stack([rows[k] for k in ("red", "green", "blue")], axis=-1), rgb)


def test_save_ply_float_colours_follow_the_reference_rule(tmp_path):
    from unidepth_amd import save_ply
    xyz = np.zeros((2, 3), np.float32)
    save_ply(str(tmp_path / "a.ply"), xyz, np.array([[0.0, 0.5, 1.0], [1.0, 0.25, 0.0]], np.float32))
    _, _, props, off = _read_ply(tmp_path / "a.ply")
    rows = np.fromfile(tmp_path / "a.ply", dtype=np.dtype([(n, "<f4" if t == "float" else "u1") for t, n in props]), offset=off)
    assert rows["red"].tolist() == [0, 255] and rows["green"].tolist() == [127, 63] and rows["blue"].tolist() == [255, 0]
    with pytest.raises(ValueError):
        save_ply(str(tmp_path / "b.ply"), np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        save_ply(str(tmp_path / "b.ply"), xyz, np.zeros((3, 3), np.uint8))


def test_save_file_ply_is_the_reference_format(tmp_path):
    from unidepth_amd import save_file_ply
    xyz = np.array([[1.5, -2.25, 3.0], [0.0, 0.0, 0.0], [-10.125, 100.0, 1e-7]], dtype=np.float64)
    rgb = np.array([[0.0, 0.5, 1.0], [0.2, 0.4, 0.6], [1.0, 0.0, 0.25]], dtype=np.float32)      # max < 1.001: scaled by 255
    path = tmp_path / "cloud_ascii.ply"
    save_file_ply(xyz, rgb, str(path))
    lines = path.read_text().splitlines()
    assert lines[:9] == ["ply", "format ascii 1.0", "element vertex 3", "property float x", "property float y", "property float z",
                         "property uchar red", "property uchar green", "property uchar blue"]
    assert lines[9] == "end_header" and len(lines) == 13
    assert lines[10] == "  1.500000  -2.250000   3.000000 0 127 255"
    assert lines[12] == "-10.125000 100.000000   0.000000 255 0 63"
    save_file_ply(xyz, np.array([[0, 128, 255]] * 3, dtype=np.uint8), str(path))             # max >= 1.001: taken as 0..255
    assert path.read_text().splitlines()[10] == "  1.500000  -2.250000   3.000000 0 128 255"


# ---- pack_points argument errors (CPU tensors: every check comes before any launch) ---------------------------------------------------

def test_pack_points_argument_errors():
    from unidepth_amd import from_prediction, pack_points
    pts = torch.zeros(2, 3, 6, 8)
    dep = torch.ones(2, 1, 6, 8)
    K = torch.eye(3)
    bad = [
        dict(),                                                                   # neither points nor depth
        dict(points=pts, mask=torch.ones(2, 1, 6, 9, dtype=torch.bool)),          # shape mismatch
        dict(points=pts, depth=torch.ones(2, 1, 8, 6)),
        dict(points=pts, image=torch.zeros(2, 3, 6, 7, dtype=torch.uint8)),
        dict(points=torch.zeros(2, 4, 6, 8)),
        dict(points=pts, confidence=torch.ones(1, 1, 6, 8), min_confidence=0.5),
        dict(points=pts, min_confidence=0.5),                                     # min_confidence without confidence
        dict(depth=dep),                                                          # depth without intrinsics
        dict(depth=dep, intrinsics=torch.eye(3).expand(3, 3, 3)),                 # nK not 1 or B
        dict(points=pts, depth_range=5.0),                                        # not a pair
        dict(points=pts, depth_range=(1.0, 2.0, 3.0)),
        dict(points=pts.double()),                                                # dtypes
        dict(points=pts, mask=torch.ones(2, 6, 8)),
        dict(points=pts, image=torch.zeros(2, 3, 6, 8, dtype=torch.float16)),
        dict(points=pts, capacity=-1),
        dict(points=pts),                                                         # a CPU tensor: there is no CPU path
        dict(depth=dep, intrinsics=K),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            pack_points(**kw)
    with pytest.raises(ValueError):
        from_prediction({"depth": dep})
    # capacity and workspace are judged before anything asks for a GPU, each in its own sentence: a bool is no capacity; the workspace is
    # a tensor, 8-byte aligned
    odd = torch.empty(1 << 16, dtype=torch.uint8)[1:]
    assert odd.data_ptr() % 8
    for kw, what in ((dict(capacity=True), "capacity"), (dict(workspace=bytearray(1 << 16)), "workspace"), (dict(workspace=odd), "workspace")):
        with pytest.raises(ValueError, match=f"pack_points: {what} must be"):
            pack_points(points=pts, **kw)
