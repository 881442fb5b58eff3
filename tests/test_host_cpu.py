"""CPU-side checks: the C-ABI library loads and exports every symbol include/unidepth_hip.h declares (no compute
without a GPU), the ctypes mirror matches the header, host logic (shape policy, weight repacking algebra,
checkpoint round trip) agrees with the oracle."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dry_run():
    """tests/dry_run.py: the host recording context and the models with host-packed weights."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dry_run", os.path.join(ROOT, "tests", "dry_run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_header_symbols():
    import ctypes
    from unidepth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unidepth_hip.h")).read()
    names = set(re.findall(r"\b(ud_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 28
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in sorted(names):
        assert hasattr(lib, n), f"libunidepth_hip.so does not export {n}"
    assert _lib.lib.ud_version() >= 100


def test_bad_arguments_fail_loudly_without_gpu():
    from unidepth_amd import ops
    import ctypes as C
    d = ops.mk(ops.UdGemm, M=128, N=128, K=100)           # null pointers, K % 64 != 0
    rc = ops.lib.ud_gemm_f16(C.byref(d), None)
    assert rc < 0 and b"bad argument" in ops.lib.ud_last_error()
    with pytest.raises(RuntimeError):
        ops.check(rc, "ud_gemm_f16")


def test_engine_requires_gpu_and_has_no_cpu_path():
    from oracle import synth
    from unidepth_amd import UniDepthV2
    cfg = synth.load_config("vits14")
    m = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, 1))
    with pytest.raises(RuntimeError, match="GPU"):
        m.infer(torch.zeros(3, 28, 28, dtype=torch.uint8))


def test_shape_policy_matches_oracle():
    from oracle import restate
    from unidepth_amd import unidepthv2 as u
    import random
    rnd = random.Random(0)
    for _ in range(500):
        H, W = rnd.randint(60, 2000), rnd.randint(60, 2000)
        assert u.get_paddings((H, W), (0.5, 2.5)) == restate.get_paddings((H, W), (0.5, 2.5))
        padded = u.get_paddings((H, W), (0.5, 2.5))[1]
        for rng in ((200000, 600000), (240000.0, 280000.0)):
            assert u.get_resize_factor(padded, rng) == restate.get_resize_factor(padded, rng)


def test_weight_folding_algebra_matches_oracle_blocks():
    """LayerNorm/LayerScale folding + head padding reproduce the oracle's block arithmetic in fp32 (before fp16 rounding)."""
    from oracle import restate, synth
    from unidepth_amd import weights
    import torch.nn.functional as F
    cfg = synth.load_config("vitb14")          # 48-wide decoder heads -> exercises head padding
    sd = synth.make_synthetic_checkpoint(cfg, 5)
    w = weights.pack(cfg, sd, "cpu")
    a = weights.arch_of(cfg)
    D, C, H = a["D"], a["C"], a["dec_heads"]
    x = torch.randn(5, D)
    # encoder qkv with folded norm1
    ref = F.linear(F.layer_norm(x, (D,), sd["pixel_encoder.blocks.3.norm1.weight"], sd["pixel_encoder.blocks.3.norm1.bias"], 1e-6),
                   sd["pixel_encoder.blocks.3.attn.qkv.weight"], sd["pixel_encoder.blocks.3.attn.qkv.bias"])
    got = F.linear(F.layer_norm(x, (D,), eps=1e-6), w["enc.3.qkv.w"].float()[:, :D], w["enc.3.qkv.b"])
    qc = (D // a["heads"]) ** -0.5 * weights.LOG2E         # the q rows carry the softmax scale and log2(e) (UdAttention.q_prescaled)
    got[:, :D] /= qc
    assert (got - ref).norm() / ref.norm() < 2e-3          # fp16 weight rounding only
    # decoder cross-attention block 1 end to end on a tiny problem, fp32 activations
    orc = restate.OracleV2(cfg, sd)
    xq, ctx = torch.randn(2, 7, C), torch.randn(2, 5, C)
    want = orc._attn_block(xq, "pixel_decoder.depth_layer.prompt_camera.1.layers.0", context=ctx, layer_scale=False)
    g = lambda name: w["dhg." + name][1]          # block 1 of the stacked (grouped-launch) weights
    hd = C // H
    q = F.linear(F.layer_norm(xq, (C,), eps=1e-5), g("q.w").float()[:, :C], g("q.b")).view(2, 7, H, 64).transpose(1, 2)
    kv = F.linear(F.layer_norm(ctx, (C,), eps=1e-5), g("kv.w").float()[:, :C], g("kv.b"))
    k = kv[..., : H * 64].view(2, 5, H, 64).transpose(1, 2)
    v = kv[..., H * 64:].view(2, 5, H, 64).transpose(1, 2)
    o = torch.softmax(q @ k.transpose(-1, -2) / weights.LOG2E, -1) @ v       # q already holds hd^-1/2 * log2(e)
    y = xq + F.linear(o.transpose(1, 2).reshape(2, 7, H * 64), g("out.w").float())
    hmid = F.gelu(F.linear(F.layer_norm(y, (C,), eps=1e-5), g("fc1.w").float(), g("fc1.b")))
    y = y + F.linear(hmid, g("fc2.w").float(), g("fc2.b"))
    assert (y - want).norm() / want.norm() < 3e-3


def test_checkpoint_roundtrip(tmp_path):
    from oracle import synth
    from unidepth_amd import UniDepthV2
    cfg = synth.load_config("vits14")
    sd = synth.make_synthetic_checkpoint(cfg, 3)
    m = UniDepthV2(cfg).load_state_dict({"module." + k: v for k, v in sd.items()})     # DDP prefix is stripped (unidepthv2.py:388)
    m.save_pretrained(str(tmp_path))
    m2 = UniDepthV2.from_pretrained(str(tmp_path))
    assert m2.config == cfg
    sd2 = m2.state_dict()
    assert set(sd2) == set(sd) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_camera_bookkeeping_matches_oracle():
    """unidepth_amd.cameras.network_params (pad = crop by negative offsets, then resize) against the oracle's restatement of the
    reference bookkeeping, for a padded + resized Spherical case and an EUCM case; reference-class look-alikes are accepted by name."""
    import torch
    from oracle import restate
    from unidepth_amd import cameras
    pads, rf = (0, 0, 12, 12), 1.3571428
    sp = cameras.Spherical(torch.tensor([0.0, 0.0, 0.0, 0.0, 560.0, 200.0, 1.4, 0.5]))
    p = sp.network_params(pads, rf)[0]
    assert abs(p[4].item() - 560.0 * rf) < 1e-3 and abs(p[5].item() - 224.0 * rf) < 1e-3
    assert abs(p[7].item() - 0.5 * 224.0 / 200.0) < 1e-6 and abs(p[6].item() - 1.4) < 1e-6 and abs(p[3].item() - 12 * rf) < 1e-4
    assert sp.params[0, 5].item() == 200.0                                   # the caller's object is not modified
    eu = cameras.EUCM(torch.tensor([190.0, 192.0, 203.0, 148.0, 0.62, 1.08]))
    q = eu.network_params((3, 4, 0, 0), 0.5)[0]
    assert torch.allclose(q, torch.tensor([95.0, 96.0, 103.0, 74.0, 0.62, 1.08]))

    class EUCM:                                                              # stands in for unidepth.utils.camera.EUCM
        def __init__(self, params):
            self.params = params
    w = cameras.as_camera(EUCM(torch.tensor([[190.0, 192.0, 203.0, 148.0, 0.62, 1.08]])))
    assert isinstance(w, cameras.EUCM) and w.gt_mode == cameras.GT_EUCM

    class MEI:                                                               # iterative models are matched by name as well
        params = torch.tensor([[150.0, 151.0, 98.0, 70.0, -0.1, 0.02, 1e-3, -1e-3, 0.9]])
    m = cameras.as_camera(MEI())
    assert m.gt_mode == cameras.GT_MEI and torch.allclose(m.network_params((2, 2, 0, 0), 2.0)[0, :4], torch.tensor([300.0, 302.0, 200.0, 140.0]))

    class Kannala:
        params = torch.zeros(1, 8)
    import pytest
    with pytest.raises(NotImplementedError):
        cameras.as_camera(Kannala())
    with pytest.raises(AssertionError):                                      # OPENCV's rational (poly-division) terms are rejected, as in the reference
        cameras.OPENCV(torch.tensor([180.0, 180, 98, 70, -0.2, 0.05, 0, 0.01, 0, 0, 0, 0, 0, 0, 0, 0]))
    with pytest.raises(AssertionError):                                      # one camera per call for the iterative models
        cameras.Fisheye624(torch.zeros(2, 16))
    # the oracle's rays for the padded Spherical case are unit vectors pointing forward at the image centre
    r = restate.OracleV2._rays_from_camera_model("Spherical", torch.tensor([0.0, 0.0, 0.0, 0.0, 560.0, 200.0, 1.4, 0.5]), pads, rf, 304, 760)
    assert torch.allclose(r.norm(dim=1), torch.ones(1, 304, 760), atol=1e-6) and r[0, 2, 152, 380] > 0.99


def test_hubconf_at_repo_root():
    """torch.hub layout: hubconf.py at the repo root exposes UniDepth and its dependency list (reference hubconf.py:1,25)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hubconf.py")
    spec = importlib.util.spec_from_file_location("ud_hubconf", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.UniDepth) and "torch" in mod.dependencies
    m = mod.UniDepth(version="v2", backbone="vitb14", pretrained=False)
    assert type(m).__name__ == "UniDepthV2"


def test_hub_entry_point_surface():
    """hubconf.UniDepth(version, backbone, pretrained) signature (reference hubconf.py:25-41): V2 configs resolve, v1 / cnvnxtl and
    v1 / vitl14 build the engine's UniDepthV1, v2old fails loudly."""
    import pytest
    import unidepth_amd
    m = unidepth_amd.UniDepth(version="v2", backbone="vits14", pretrained=False)
    assert type(m).__name__ == "UniDepthV2" and m.shape_constraints["pixels_max"] > m.shape_constraints["pixels_min"]
    with pytest.raises(AssertionError):
        unidepth_amd.UniDepth(version="v2", backbone="cnvnxtl", pretrained=False)
    m1 = unidepth_amd.UniDepth(version="v1", backbone="cnvnxtl", pretrained=False)
    assert type(m1).__name__ == "UniDepthV1" and m1.image_shape == [462, 616] and len(m1.embed_dims) == 36 and m1.depths == [3, 6, 33, 36]
    m2 = unidepth_amd.UniDepth(version="v1", backbone="vitl14", pretrained=False)
    assert type(m2).__name__ == "UniDepthV1" and len(m2.embed_dims) == 24 and m2.depths == [5, 12, 18, 24] and m2.patch_size == 14 and m1.patch_size == 16
    with pytest.raises(NotImplementedError):
        unidepth_amd.UniDepth(version="v2old", backbone="vitl14", pretrained=False)
    with pytest.raises(RuntimeError):
        m1.pixel_encoder(torch.zeros(1, 3, 64, 64))           # no weights / not on a GPU: fails loudly, no CPU path


def test_plan_cache_is_an_lru_and_state_resets(monkeypatch):
    """The per-(batch, shape, camera, slot) plan cache is bounded and load_state_dict / to() drop every derived cache."""
    import collections
    from unidepth_amd.unidepthv2 import UniDepthV2
    from oracle import synth
    cfg = synth.load_config("vits14")
    m = UniDepthV2(cfg)
    m.resolution_level = 0
    m.max_plans = 3
    import unidepth_amd.unidepthv2 as U
    made = []

    class _P:
        def __init__(self, model, B, H, W, *a):
            made.append((B, H, W))
    monkeypatch.setattr(U, "_Plan", _P)
    monkeypatch.setattr(U.torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    for hw in [(10, 10), (20, 20), (30, 30), (10, 10), (40, 40), (20, 20)]:
        m._plan(1, hw[0], hw[1], 0, True, True)
    assert isinstance(m._plans, collections.OrderedDict) and len(m._plans) == 3
    # (10,10) was refreshed before (40,40) evicted the oldest -> (20,20) had to be rebuilt, (10,10) not
    assert made == [(1, 10, 10), (1, 20, 20), (1, 30, 30), (1, 40, 40), (1, 20, 20)]
    m._pos_cache[(3, 3)] = torch.zeros(1)
    m.load_state_dict({"module.x": torch.zeros(1)})
    assert len(m._plans) == 0 and len(m._pos_cache) == 0
    m.clear_plans()


def test_arch_of_rejects_unsupported_encoder_settings():
    import copy
    from unidepth_amd.weights import arch_of
    from oracle import synth
    cfg = synth.load_config("vits14")
    arch_of(cfg)
    bad = copy.deepcopy(cfg)
    bad["model"]["pixel_encoder"]["use_norm"] = False
    with pytest.raises(NotImplementedError):
        arch_of(bad)
    bad = copy.deepcopy(cfg)
    bad["model"]["pixel_encoder"]["stacking_fn"] = "sum"
    with pytest.raises(NotImplementedError):
        arch_of(bad)


def test_product_library_has_no_debug_switches():
    """ud_set_debug_flags changed product numerics in round 1; it now exists only in instrumented tools builds (-DUD_TOOLS)."""
    import ctypes
    from unidepth_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert not hasattr(lib, "ud_set_debug_flags")


def test_eval_ops_argument_checks_mirror_the_reference_and_refuse_cpu_tensors():
    """knn_points / ChamferDistance / RandomPatchExtractor (unidepth_amd/eval_ops.py): the reference's ValueErrors
    (functions/knn.py:170-173,70; chamfer_distance.py:16-30,49-53) and no CPU path."""
    import pytest
    import torch
    from unidepth_amd import eval_ops
    a = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="same batch dimension"):
        eval_ops.knn_points(a, torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match="same point dimension"):
        eval_ops.knn_points(a, torch.zeros(1, 4, 2))
    with pytest.raises(ValueError, match="1 or 2 norm"):
        eval_ops.knn_points(a, a, norm=3)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        eval_ops.knn_points(a, a)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        eval_ops.RandomPatchExtractor()(torch.zeros(1, 1, 8, 8), torch.zeros(1, 2, 2), (3, 3))
    cd = eval_ops.ChamferDistance()
    with pytest.raises(ValueError, match="batch_reduction"):
        cd(a, a, batch_reduction="max")
    with pytest.raises(ValueError, match="point_reduction"):
        cd(a, a, point_reduction="max")
    with pytest.raises(ValueError, match="shape"):
        cd(torch.zeros(4, 3), a)
    with pytest.raises(ValueError, match="lengths"):
        cd(a, a, x_lengths=torch.zeros(2, dtype=torch.int64))
    idx = torch.tensor([[[1, 0], [2, 2]]])
    x = torch.arange(6.0).view(1, 3, 2)
    g = eval_ops.knn_gather(x, idx, lengths=torch.tensor([1]))          # slots k >= length are zero (functions/knn.py:238-247)
    assert torch.equal(g[0, :, 0], x[0, [1, 2]]) and float(g[0, :, 1].abs().sum()) == 0.0


def test_v1_host_shape_policy_and_position_embedding_match_the_oracle():
    """UniDepthV1's integer shape policy (unidepthv1.py:29-47 _paddings / _shapes) and the sine position embedding constant
    (layers/positional_encoding.py:14-57) on the engine's host side vs the restatement that is pinned on the reference."""
    import torch
    from oracle import restate_v1
    from unidepth_amd import unidepthv1 as v1
    for img in ((480, 640), (200, 360), (240, 320), (375, 1242), (1080, 1920), (500, 333), (31, 977), (462, 616)):
        for net in ((462, 616), (480, 640)):
            a, b = v1.v1_shapes(img, net), restate_v1.v1_shapes(img, net)
            assert a[0] == b[0] and a[2] == b[2] and abs(a[1] - b[1]) < 1e-12, (img, net, a, b)
            (nh, nw), _, (pl, pr, pt, pb) = a
            assert nh + pt + pb == net[0] and nw + pl + pr == net[1] and min(pl, pr, pt, pb) >= 0
    for (h, w, npf) in ((30, 40, 256), (29, 39, 256), (15, 20, 64)):
        a, b = v1.pos_embed_sine(h, w, npf), restate_v1.pos_embed_sine(h, w, npf)
        assert a.shape == b.shape and torch.allclose(a.reshape(-1), b.reshape(-1), atol=1e-6, rtol=0)


def test_v1_split_weight_packing_is_exact_to_22_bits():
    """UniDepthV1 weights as two fp16 terms (unidepthv1._padk16 / _conv3_rows / _wk / _ak): W_hi + W_lo reproduces the fp32 weight to ~2^-22,
    the K concatenation has the layout the kernels' wrap-around loaders expect (dense: [hi(Kp) | lo(Kp)], 3x3: per tap [hi(Cin) | lo(Cin)]),
    and the descriptor helpers derive K / a_wrap / Cin from the packed width."""
    from unidepth_amd import unidepthv1 as U
    g = torch.Generator().manual_seed(0)
    w = torch.randn(96, 200, generator=g) * 200 ** -0.5
    p = U._padk16(w, split=True)
    assert p.shape == (96, 512) and p.dtype == torch.float16
    hi, lo = p[:, :200].float(), p[:, 256:456].float()
    assert (p[:, 200:256] == 0).all() and (p[:, 456:] == 0).all()
    assert torch.equal(hi, w.half().float())
    err = ((hi + lo) - w).abs().max() / w.abs().max()
    assert err < 2 ** -20, float(err)
    assert ((w.half().float() - w).abs().max() / w.abs().max()) > 100 * err          # the single term carries the 2^-11 rounding
    assert U._wk(p, 256) == dict(K=512, ldw=512, a_wrap=256) and U._wk(U._padk16(w, split=False), 256) == dict(K=256, ldw=256)
    assert U._ak(p, 256) == dict(K=512, lda=512, w_wrap=256)
    wc = torch.randn(32, 64, 3, 3, generator=g) * 576 ** -0.5
    rows = U._conv3_rows(wc, split=True)                                     # fp32 [Cout, 9 * 2 * Cin], exactly representable halves
    assert rows.shape == (32, 9 * 128)
    r = rows.view(32, 9, 2, 64)
    want = wc.permute(0, 2, 3, 1).reshape(32, 9, 64)
    assert torch.equal(r[:, :, 0], want.half().float()) and ((r[:, :, 0] + r[:, :, 1]) - want).abs().max() < 2 ** -20 * want.abs().max()
    assert torch.equal(rows.half().float(), rows)                                # the later fp16 cast is exact
    pk = U._padk16(rows, split=False)
    assert U._wk(pk, 0, 64) == dict(K=pk.shape[1], ldw=pk.shape[1], Cin=128, a_wrap=64)
    assert U._wk(U._padk16(U._conv3_rows(wc, split=False), split=False), 0, 64)["Cin"] == 64


def test_v1_three_term_product_layout_removes_the_activation_rounding():
    """Round 4: the ConvUpsample tails and output convs of UniDepthV1 multiply [A_hi | A_lo] with [W_hi | W_hi | W_lo], the
    A index wrapping once after 2 K columns / 2 Cin channels (UdGemm.a_wrap).  Emulated here exactly as the kernels walk K (fp16 operands,
    wide accumulate): the product matches the fp32 one to ~2^-21 where the two-term product ([A_hi] x [W_hi | W_lo]) keeps the 2^-11
    activation rounding; the descriptor helper derives the fields from the packed width; the packed decoder uses the layout where the
    seed study put the error."""
    from unidepth_amd import unidepthv1 as U
    g = torch.Generator().manual_seed(1)
    M, N, K = 40, 24, 128
    a = torch.randn(M, K, generator=g) * (1.0 + 3.0 * torch.rand(1, K, generator=g))           # channels of unequal scale, non-zero mean
    a += 2.0
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w3 = U._padk16_3(w)
    assert w3.shape == (N, 3 * K) and U._wk(w3, K) == dict(K=3 * K, ldw=3 * K, a_wrap=2 * K)
    a_hi = a.half()
    a2 = torch.cat([a_hi, (a - a_hi.float()).half()], dim=1)                                  # what UD_V1_COPY_ROWS to_f16 = 2 writes
    ka = torch.arange(3 * K)
    ka = torch.where(ka >= 2 * K, ka - 2 * K, ka)                                              # the loader's wrap
    y3 = a2[:, ka].double() @ w3.double().t()
    ref = a.double() @ w.double().t()
    w2 = U._padk16(w, split=True)
    y2 = torch.cat([a_hi, a_hi], dim=1).double() @ w2.double().t()
    e3, e2 = (y3 - ref).abs().max() / ref.abs().max(), (y2 - ref).abs().max() / ref.abs().max()
    assert e3 < 2e-6 and e2 > 20 * e3, (float(e3), float(e2))
    # 3x3: per tap [W_hi | W_hi | W_lo] against an image of 2 Cin channels
    wc = torch.randn(8, 16, 3, 3, generator=g) * 144 ** -0.5
    rows = U._conv3_rows_3(wc)
    assert rows.shape == (8, 9 * 48) and torch.equal(rows.half().float(), rows)
    r = rows.view(8, 9, 3, 16)
    want = wc.permute(0, 2, 3, 1).reshape(8, 9, 16)
    assert torch.equal(r[:, :, 0], r[:, :, 1]) and torch.equal(r[:, :, 0], want.half().float())
    assert ((r[:, :, 0] + r[:, :, 2]) - want).abs().max() < 2 ** -20 * want.abs().max()
    pk = U._padk16(U._conv3_rows_3(torch.randn(8, 64, 3, 3, generator=g)), split=False)
    assert U._wk(pk, 0, 64) == dict(K=pk.shape[1], ldw=pk.shape[1], Cin=192, a_wrap=128)
    # the packed decoder: three-term layout on up*.up.0 / up*.up.2, two-term elsewhere
    from oracle import synth_v1
    assert U.ASPLIT
    cfg = synth_v1.load_config_v1()
    C = cfg["model"]["pixel_decoder"]["hidden_dim"]
    wd = U.pack_v1_decoder(cfg, synth_v1.make_synthetic_checkpoint_v1(cfg, 211), torch.device("cpu"))
    for nm, d in (("up8", C), ("up4", C // 2), ("up2", C // 4)):
        assert wd[f"{nm}.up0.w"].shape == (d // 2, 3 * d) and U._wk(wd[f"{nm}.up0.w"], d)["a_wrap"] == 2 * d
        assert U._wk(wd[f"{nm}.up2.w"], 0, d // 2) == dict(K=27 * (d // 2), ldw=27 * (d // 2), Cin=3 * (d // 2), a_wrap=d)
        assert U._wk(wd[f"{nm}.0.fc2.w"], 4 * d)["a_wrap"] == 4 * d                         # the CvnxtBlocks in front keep two terms
    sd = synth_v1.make_synthetic_checkpoint_v1(cfg, 211)
    for nm, d in (("out8", C // 2), ("out4", C // 4), ("out2", C // 8)):
        # the three one-channel output convs are an fp32 stencil (UD_V1_OUT_CONV3): weights [tap = ky * 3 + kx, c], the bias on the host
        wt = sd[f"pixel_decoder.depth_layer.{nm}.weight"]
        assert wd[f"{nm}.cw"].shape == (9, d) and wd[f"{nm}.cw"].dtype == torch.float32
        assert torch.equal(wd[f"{nm}.cw"][4], wt[0, :, 1, 1].float()) and torch.equal(wd[f"{nm}.cw"][2], wt[0, :, 0, 2].float())
        assert wd[f"host.{nm}.bias"] == float(sd[f"pixel_decoder.depth_layer.{nm}.bias"][0]) and f"{nm}.w" not in wd


def test_v1_every_gemm_weight_is_two_terms_by_default():
    """Default placement since round 4: every GEMM weight of the ConvNeXt encoder is [W_hi | W_lo], the blocks' fc1 included (the
    round-3 placement kept them single fp16 for -6.9 % time; over the 8-seed sweep that was a global depth shift of up to 8.6e-4 and the one
    case above the bar); `_padk16(split=False)` is what UNIDEPTH_V1_WSPLIT=1 would pack for them."""
    from unidepth_amd import unidepthv1 as U
    from oracle import synth_v1
    cfg = synth_v1.load_config_v1()
    assert U.WSPLIT and U.WSPLIT_CONVNEXT_FC1 and U.ASPLIT                        # the environment of the test run: defaults
    w = U.pack_convnext(cfg, synth_v1.make_synthetic_checkpoint_v1(cfg, 211), torch.device("cpu"))
    dims = U.CONVNEXT[cfg["model"]["pixel_encoder"]["name"]]["dims"]
    for s, C in enumerate(dims):
        assert w[f"blk.{s}.0.fc1.w"].shape == (4 * C, 2 * C) and U._wk(w[f"blk.{s}.0.fc1.w"], C) == dict(K=2 * C, ldw=2 * C, a_wrap=C)
        assert w[f"blk.{s}.0.fc2.w"].shape == (C, 8 * C) and U._wk(w[f"blk.{s}.0.fc2.w"], 4 * C)["a_wrap"] == 4 * C
    assert w["ds.1.w"].shape[1] == 2 * 4 * dims[0] and w["stem.w"].shape[1] == 128
    assert U._wk(U._padk16(torch.zeros(8, dims[0]), split=False), dims[0]) == dict(K=dims[0], ldw=dims[0])


def test_v1_nystrom_block_fused_kv_packing():
    """The decoder packer stores ONE [K | V] weight per NystromBlock (K rows first, as the reference's `kv` Linear + 'b n (kv h d)' rearrange
    orders them, layers/nystrom_attention.py:59-62) with the context LayerNorm folded in."""
    from unidepth_amd import unidepthv1 as U
    from oracle import synth_v1
    cfg = synth_v1.load_config_v1()
    sd = synth_v1.make_synthetic_checkpoint_v1(cfg, 211)
    w = U.pack_v1_decoder(cfg, sd, torch.device("cpu"))
    C = cfg["model"]["pixel_decoder"]["hidden_dim"]
    for nm, d in (("layers_8", C // 2), ("layers_4", C // 4)):
        kv = w[f"{nm}.0.kv.w"]
        assert kv.shape == (2 * d, 2 * d) and f"{nm}.0.k.w" not in w                 # [K | V] rows, two fp16 terms along K
        src = f"pixel_decoder.depth_layer.{nm}.0."
        g = sd[src + "norm_attnctx.weight"].float()
        want = sd[src + "kv.weight"].float() * g[None, :]
        got = kv[:, :d].float() + kv[:, d:].float()
        assert (got - want).abs().max() < 2 ** -20 * want.abs().max()


def test_v1_vit_position_embedding_scale_factor_form():
    """UniDepthV1 builds its DINOv2 with interpolate_offset = 0.1: the position embedding is resampled with scale factors (h + 0.1) / 37, not
    with an output size (backbones/dinov2.py:283-296) -- the engine's host-side resample against the pinned oracle's, and against the V2 form
    (they must differ: a silent swap would cost ~1e-2 in the tokens)."""
    from oracle import restate_v1, synth_v1
    from unidepth_amd.unidepthv1 import vit_pos_embed_v1
    cfg = synth_v1.load_config_v1("vitl14")
    pe = torch.randn(1, 37 * 37 + 1, 64, generator=torch.Generator().manual_seed(1))
    orc = restate_v1.OracleV1.__new__(restate_v1.OracleV1)
    orc.w = {"pixel_encoder.pos_embed": pe}
    want = orc._vit_pos_embed(33, 44)[0]
    got = vit_pos_embed_v1(pe, 33, 44)
    assert got.shape == (33 * 44 + 1, 64) and torch.allclose(got, want, atol=1e-6)
    grid = pe[:, 1:].reshape(1, 37, 37, 64).permute(0, 3, 1, 2)
    v2 = torch.nn.functional.interpolate(grid, size=(33, 44), mode="bicubic", antialias=False).permute(0, 2, 3, 1).reshape(33 * 44, 64)
    assert (got[1:] - v2).abs().max() > 1e-3
    assert torch.equal(vit_pos_embed_v1(pe, 37, 37), pe[0])


def test_engine_classes_are_nn_modules(tmp_path):
    """Reference: `class UniDepthV2(nn.Module, PyTorchModelHubMixin, ...)` (unidepthv2.py:111-117; V1: unidepthv1.py:97-103).  Code written
    against it may type-check, call, cast or walk the model: the engine classes answer those calls (unidepth_amd/module.py) -- no
    registered parameters (weights live as repacked device buffers), casts are warned no-ops, train(True) is refused, state_dict() is the
    fp32 reference-keyed dict, save_pretrained / from_pretrained round-trip in the HF layout, push_to_hub exists with huggingface_hub."""
    import warnings
    import torch
    from oracle import synth, synth_v1
    from unidepth_amd import UniDepthV1, UniDepthV2
    from unidepth_amd.export import UniDepthV2ONNX
    cfg = synth.load_config("vits14")
    sd = synth.make_synthetic_checkpoint(cfg, 3)
    for cls in (UniDepthV2, UniDepthV2ONNX):
        m = cls(cfg).load_state_dict(sd)
        assert isinstance(m, torch.nn.Module) and list(m.parameters()) == [] and m.training is False
        assert m.eval() is m and m.train(False) is m and m.requires_grad_(False) is m and m.cpu() is m
        with pytest.raises(RuntimeError):
            m.train()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert m.half() is m and m.float() is m and m.bfloat16() is m and m.to(torch.float16) is m and m.to(dtype=torch.float32) is m
        assert len(w) == 5 and all("no-op" in str(x.message) for x in w)
        got = m.state_dict()
        assert set(got) == set(sd) and all(got[k].dtype == torch.float32 and torch.equal(got[k], sd[k].float()) for k in sd)
        with pytest.raises(RuntimeError, match="ROCm GPU only"):        # model(...) is infer(): no CPU path, and it says so
            m(torch.zeros(1, 3, 28, 28))
    m.save_pretrained(tmp_path / "v2")
    m2 = UniDepthV2.from_pretrained(str(tmp_path / "v2"))
    assert all(torch.equal(m2.state_dict()[k], got[k]) for k in got) and m2.config == cfg
    try:
        import huggingface_hub  # noqa: F401
        assert callable(getattr(m, "push_to_hub", None))
    except ImportError:
        pass
    cfg1 = synth_v1.load_config_v1("cnvnxtl")
    v1 = UniDepthV1(cfg1)
    assert isinstance(v1, torch.nn.Module) and v1.eval() is v1 and v1.device.type == "cpu"


def test_v1_plan_builder_dry_run_validates_every_gemm_descriptor():
    """The launch program of a UniDepthV1 infer() is RECORDED on the host (host tensors stand in for the device buffers, nothing runs) and
    every GEMM descriptor it records is handed to ud_gemm_f16: without a GPU the call must get past the C side's argument validation
    (wrap / K / Cin / stride rules, include/unidepth_hip.h UdGemm) and fail only at the launch itself -- a builder bug (e.g. a three-term
    weight against a two-term A stride) is caught here, not on the GPU box."""
    from unidepth_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    dry = _dry_run()
    m = dry.v1_model("cnvnxtl", 301)
    seen = []

    def add(real_add, h, dref):
        rc = _lib.lib.ud_gemm_f16(dref, None)
        seen.append((rc, _lib.lib.ud_last_error().decode() if rc else "", dref._obj.M, dref._obj.N, dref._obj.K, dref._obj.a_wrap, dref._obj.Cin))
        return real_add(h, dref)
    with dry.host_recording({"gemm": add}):
        plan = m._full_plan(1, 240, 320, True, False, True, 0, False)
    assert len(plan.prog) > 300 and len(seen) > 150      # (round 5: the NystromBlocks lost their ~90 landmark / pseudo-inverse launches)
    bad = [r for r in seen if r[0] != -2]                     # -2 = UD_ERR_LAUNCH (include/unidepth_hip.h)
    assert not bad, bad[:3]                                    # UD_ERR_BAD_ARG would mean a descriptor the kernels refuse
    three = [r for r in seen if r[5] and (3 * r[5] == 2 * r[4] or (r[6] and 3 * r[5] == 2 * r[6]))]
    assert len(three) == 6, three                              # up{8,4,2}.up.0, up{8,4,2}.up.2 (out{8,4,2} are an fp32 stencil since round 5)


def test_v2_plan_builder_dry_run_order_and_descriptors(monkeypatch):
    """The UniDepthV2 launch program recorded on the host (nothing runs): every GEMM descriptor passes the C side's argument validation, and
    the decoder starts with the grouped feature adapters, then the camera head + rays + ray embedding, then LayerNorm / q projection and the
    K / V projection of the ray embedding."""
    from unidepth_amd import _lib, ops
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    dry = _dry_run()
    m = dry.v2_model("vits14", 3, 2)
    seen = []

    def add(real_add, h, dref):
        rc = _lib.lib.ud_gemm_f16(dref, None)
        seen.append((rc, _lib.lib.ud_last_error().decode() if rc else ""))
        return real_add(h, dref)
    with dry.host_recording({"gemm": add}):
        plan = m._plan(1, 462, 616, 0, True, True)
    assert len(seen) > 60 and not [r for r in seen if r[0] != -2], [r for r in seen if r[0] != -2][:3]     # -2 = UD_ERR_LAUNCH: arguments accepted
    tags = [t[1] for t in plan.prog.meta]
    i0 = tags.index("dec.adapters(x4)")
    assert plan.dec_first == plan.enc_last == i0
    cam = tags[i0 + 1:tags.index("ray_embed") + 1]
    # the token adapters and the CameraHead are ONE launch (UdCameraHead); its descriptor is inside the kernel's limits for every backbone
    assert cam.count("cam.head") == 1 and cam[-2:] == ["rays", "ray_embed"] and "camera_intrinsics" in cam and not any(t.startswith("dh.") for t in cam)
    assert tags[tags.index("ray_embed") + 1:tags.index("ray_embed") + 4] == ["layernorm", "dh.q(x4)", "dh.kv(x4)"]
    # outside the one-launch kernel's limits the same layers are recorded one by one (4 adapters, 14 Linears, 6 LayerNorms, 2 attentions: 26 launches)
    monkeypatch.setattr(ops, "camera_head_supported", lambda d: False)
    m.clear_plans()
    with dry.host_recording({"gemm": add}):
        plan2 = m._plan(1, 462, 616, 0, True, True)
    tags2 = [t[1] for t in plan2.prog.meta]
    cam2 = tags2[tags2.index("dec.adapters(x4)") + 1:tags2.index("ray_embed") + 1]
    assert "cam.head" not in cam2 and cam2.count("cam.adapter") == 4 and cam2.count("attention_small") == 2
    assert sum(t.startswith("cam.cam.") for t in cam2) == 14 and len(plan2.prog) == len(plan.prog) + 25


def test_program_api_argument_checks_without_gpu():
    """ud_program_run on the host: ranges are validated before anything touches the device, an empty range is a no-op."""
    from unidepth_amd import _lib
    lib = _lib.lib
    p = lib.ud_program_create()
    assert p and lib.ud_program_size(p) == 0
    assert lib.ud_program_run(p, -1, 2, None) == -1 and b"bad range" in lib.ud_last_error()
    assert lib.ud_program_run(p, 0, 1, None) == -1
    assert lib.ud_program_run(p, 0, 0, None) == 0                                                    # empty range: nothing to do
    lib.ud_program_destroy(p)


def test_camera_head_cabi_limits_without_gpu():
    """ud_camera_head_supported (host-side check of the one-launch camera head's limits, include/unidepth_hip.h UdCameraHead) and the
    argument validation of ud_camera_head_f32: refused descriptors never reach a launch."""
    import ctypes as C
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_camera_head_supported(None) == -1 and lib.ud_camera_head_f32(None, None) == -1
    x = torch.zeros(32, 2048); W = torch.zeros(2048, 2048); out = torch.zeros(32, 2048); ws = torch.zeros(16, dtype=torch.int32)

    def desc(**kw):
        d = _lib.UdCameraHead()
        d.n_phases, d.T, d.H, d.C, d.scale, d.eps, d.sync_ws = 1, 4, 8, 512, 0.125, 1e-5, ws.data_ptr()
        ph = dict(x=x.data_ptr(), W=W.data_ptr(), out=out.data_ptr(), M=32, N=512, K=512, ldx=512, ldc=512, kind=0, ln=1)
        ph.update(kw)
        for k, v in ph.items():
            setattr(d.ph[0], k, v)
        return d
    assert lib.ud_camera_head_supported(C.byref(desc())) == 0
    assert lib.ud_camera_head_supported(C.byref(desc(N=2048, ldc=2048))) == 0                      # 16 columns x 512 floats = 32 KB: the slab limit
    assert lib.ud_camera_head_supported(C.byref(desc(N=2049, ldc=2052))) == -3 and b"limits" in lib.ud_last_error()
    assert lib.ud_camera_head_supported(C.byref(desc(K=500, ldx=512))) == -3                 # K % 128
    assert lib.ud_camera_head_supported(C.byref(desc(K=1024, ldx=1024))) == -3               # LayerNorm phase with K > 512
    assert lib.ud_camera_head_supported(C.byref(desc(K=1024, ldx=1024, ln=0))) == 0
    assert lib.ud_camera_head_supported(C.byref(desc(kind=1, ldx=1536))) == 0 and lib.ud_camera_head_supported(C.byref(desc(kind=1, ldx=1024))) == -3
    assert lib.ud_camera_head_supported(C.byref(desc(x=None))) == -1
    d = desc(); d.n_phases = 25
    assert lib.ud_camera_head_supported(C.byref(d)) == -1
    d = desc(); d.sync_ws = None
    assert lib.ud_camera_head_f32(C.byref(d), None) == -1
    p = lib.ud_program_create()
    assert lib.ud_program_add_camera_head(p, C.byref(desc())) == 0 and lib.ud_program_size(p) == 1
    lib.ud_program_destroy(p)


def test_rccl_cabi_argument_checks_without_gpu():
    """ud_rccl_* (the exchange step of batch data parallelism behind the C-ABI): arguments are validated and a missing communicator is an
    error, before librccl or a device is touched."""
    from unidepth_amd import _lib
    lib = _lib.lib
    assert lib.ud_rccl_unique_id(None) == -1
    assert lib.ud_rccl_init(None, 2, 0) == -1 and lib.ud_rccl_init(b"x" * 128, 2, 2) == -1 and lib.ud_rccl_init(b"x" * 128, 0, 0) == -1
    assert lib.ud_rccl_allgather_outputs(None, None, 16, 0, None) == -1 and b"no communicator" in lib.ud_last_error()
    assert lib.ud_rccl_finalize() == 0
