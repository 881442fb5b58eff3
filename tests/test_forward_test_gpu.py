"""UniDepthV2.forward_test on the GPU (ViT-S/14, synthetic checkpoint): the reference's validation forward -- the network-resolution
plan end to end, then one ud_match_gt -- against the CPU oracle (OracleV2.encode / decode at network resolution, rays * radius, the
fp64 restatement of tools/make_golden_match_gt.py), at the bars of tests/test_parity_gpu.py::_outputs_ok."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restate, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_match_gt", os.path.join(ROOT, "tools", "make_golden_match_gt.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

B, HN, WN, H2, W2 = 2, 196, 252, 150, 201
METAS = [{"paddings": (0, 0, 0, 0)}, {"paddings": (14, 0, 28, 14)}]            # (left, top, right, bottom), as the datasets store them
PADS_LRTB = np.array([[0, 0, 0, 0], [14, 28, 0, 14]])
K_GT = torch.tensor([[[230.0, 0.0, 120.5], [0.0, 228.0, 99.0], [0.0, 0.0, 1.0]], [[250.0, 0.0, 131.0], [0.0, 251.0, 95.5], [0.0, 0.0, 1.0]]])
EUCM_PARAMS = torch.tensor([210.0, 212.0, 125.0, 97.0, 0.55, 1.1])


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unidepth_amd import UniDepthV2
    cfg = synth.load_config("vits14")
    sd = synth.make_synthetic_checkpoint(cfg, 123)
    g = torch.Generator().manual_seed(31)
    image = ((torch.rand(B, 3, HN, WN, generator=g) - 0.45) / 0.225).float()      # an already normalised network image
    model = UniDepthV2(cfg).load_state_dict(sd).to("cuda").eval()
    orc = restate.OracleV2(cfg, sd)
    with torch.no_grad():
        feats, cls = orc.encode(image)                                             # once: the three camera variants share it
    return dict(model=model, orc=orc, image=image, feats=feats, cls=cls,
                depth=torch.zeros(B, 1, H2, W2, device="cuda"))


def _inputs(s, camera=None, depth=None):
    d = {"image": s["image"].cuda(), "depth": s["depth"] if depth is None else depth}
    if camera is not None:
        d["camera"] = camera
    return d


def _pinhole_rays(K):
    """Camera.get_rays of a pinhole K at network resolution (no crop, no resize): normalise(K^-1 [u + .5, v + .5, 1])."""
    xs = torch.linspace(0.5, WN - 0.5, WN)
    ys = torch.linspace(0.5, HN - 0.5, HN)
    uv1 = torch.stack([xs.repeat(HN, 1), ys.repeat(WN, 1).t(), torch.ones(HN, WN)], 0).reshape(1, 3, -1)
    xyz = torch.inverse(K.float().reshape(-1, 3, 3)) @ uv1
    xyz = (xyz / xyz[:, -1:].clip(min=1e-4)).reshape(-1, 3, HN, WN)
    return xyz / torch.norm(xyz, dim=1, keepdim=True).clamp(min=1e-4)


def _expected(s, rays_gt):
    """The reference's forward_test restated on the CPU: decode at network resolution, points = rays * radius, the fp64 restatement
    of match_gt with image 1's paddings, match_intrinsics, network rays over their clipped norm."""
    with torch.no_grad():
        out = s["orc"].decode(s["feats"], s["cls"], HN, WN, rays_gt)
    rays = out["rays"].expand(B, 3, HN, WN)
    points = (rays * out["radius"]).numpy()
    pts = torch.from_numpy(mg.restate(points, H2, W2, PADS_LRTB, None, dtype=np.float64))
    conf = torch.from_numpy(mg.restate(out["confidence"].numpy(), H2, W2, PADS_LRTB, None, dtype=np.float64))
    K = torch.from_numpy(mg.restate_intrinsics(out["intrinsics"].numpy(), (HN, WN), (H2, W2), PADS_LRTB, None))
    return {"points": pts, "depth": pts[:, 2:], "confidence": conf, "intrinsics": K,
            "rays": rays / torch.norm(rays, dim=1, keepdim=True).clip(min=1e-5)}


def _arel(a, b):
    return ((a - b).abs() / b.abs().clamp_min(1e-6)).mean().item()


@pytest.mark.parametrize("cam", ["none", "pinhole", "eucm"])
def test_forward_test_vs_oracle(setup, cam):
    from unidepth_amd import cameras
    s = setup
    if cam == "none":
        camera, rays_gt = None, None
    elif cam == "pinhole":
        camera, rays_gt = K_GT, _pinhole_rays(K_GT)
    else:                                                                          # one non-pinhole camera for the whole batch
        camera = cameras.EUCM(EUCM_PARAMS)
        rays_gt = restate.OracleV2._rays_from_camera_model("EUCM", EUCM_PARAMS, (0, 0, 0, 0), 1.0, HN, WN)
    out = s["model"].forward_test(_inputs(s, camera), METAS)
    torch.cuda.synchronize()
    assert list(out) == ["depth", "points", "confidence", "rays", "intrinsics"]
    assert tuple(out["depth"].shape) == (B, 1, H2, W2) and tuple(out["points"].shape) == (B, 3, H2, W2)
    assert tuple(out["confidence"].shape) == (B, 1, H2, W2) and tuple(out["intrinsics"].shape) == (B, 3, 3)
    assert tuple(out["rays"].shape) == (B, 3, HN, WN)
    o = {k: v.double().cpu() for k, v in out.items()}
    for k, v in o.items():
        assert torch.isfinite(v).all(), (cam, k)
    ref = _expected(s, rays_gt)
    st = {"depth": _arel(o["depth"], ref["depth"]), "conf": _arel(o["confidence"], ref["confidence"]),
          "K": ((o["intrinsics"] - ref["intrinsics"]).abs() / ref["intrinsics"].abs().clamp_min(1.0)).max().item(),
          "rays": (o["rays"] - ref["rays"]).abs().max().item(),
          "points": ((o["points"] - ref["points"]).norm() / ref["points"].norm()).item()}
    print(cam, {k: f"{v:.2e}" for k, v in st.items()})
    assert st["depth"] <= 1e-3 and st["conf"] <= 2e-3 and st["K"] <= 2e-3 and st["rays"] <= 2e-3, (cam, st)
    # depth is the z plane of points through the same arithmetic
    assert torch.equal(out["depth"].view(torch.int32), out["points"][:, 2:].contiguous().view(torch.int32))


def test_zero_paddings_at_network_size_is_the_network_output(setup):
    """no paddings, ground truth at Hn x Wn: the matched maps are radius_net * rays_net and confidence_net bit for bit"""
    s = setup
    model = s["model"]
    out = model.forward_test(_inputs(s, depth=torch.zeros(B, 1, HN, WN, device="cuda")), [])
    taps = model.debug_taps()
    torch.cuda.synchronize()
    pts = taps["rays_net"] * taps["radius_net"].view(B, 1, HN, WN)
    assert torch.equal(out["points"].view(torch.int32), pts.view(torch.int32))
    assert torch.equal(out["depth"].view(torch.int32), pts[:, 2:].contiguous().view(torch.int32))
    assert torch.equal(out["confidence"].view(torch.int32), taps["confidence_net"].view(B, 1, HN, WN).view(torch.int32))
    assert torch.equal(out["intrinsics"], taps["intrinsics_net"])


def test_call_with_a_dict_is_forward_test(setup):
    s = setup
    a = s["model"](_inputs(s, K_GT[:1]), METAS)
    b = s["model"].forward_test(_inputs(s, K_GT[:1]), METAS)
    c = s["model"].forward(_inputs(s, K_GT[:1]), METAS)
    torch.cuda.synchronize()
    for k in b:
        assert torch.equal(a[k], b[k]) and torch.equal(c[k], b[k]), k
    # `paddings` already in (left, right, top, bottom) order in the inputs, no metas: the same result
    d = _inputs(s, K_GT[:1])
    d["paddings"] = torch.from_numpy(PADS_LRTB).cuda()
    e = s["model"].forward_test(d, [])
    for k in b:
        assert torch.equal(e[k], b[k]), k


def test_two_slots_on_two_streams_give_the_same_bits(setup):
    s = setup
    model = s["model"]
    g = torch.Generator().manual_seed(32)
    image2 = ((torch.rand(B, 3, HN, WN, generator=g) - 0.45) / 0.225).float().cuda()
    in0, in1 = _inputs(s), {"image": image2, "depth": s["depth"]}
    ref0 = model.forward_test(in0, METAS, slot=0)
    torch.cuda.synchronize()
    ref1 = model.forward_test(in1, METAS, slot=1)
    torch.cuda.synchronize()
    st0, st1 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(st0):
        out0 = model.forward_test(in0, METAS, slot=0)
    with torch.cuda.stream(st1):
        out1 = model.forward_test(in1, METAS, slot=1)
    st0.synchronize()
    st1.synchronize()
    for k in ref0:
        assert torch.equal(out0[k], ref0[k]) and torch.equal(out1[k], ref1[k]), k
    assert not torch.equal(ref0["depth"], ref1["depth"])
