"""UniDepthV1 (ConvNeXt-L backbone) on MI355X -- SURVEY.md 8f next-1, BASELINE.json configs[3] (640x480, bs=16, conv-heavy path).
Mirrors the reference class (unidepth/models/unidepthv1/unidepthv1.py:101-450): from_pretrained / to / eval / infer(rgbs, intrinsics,
skip_camera), attribute `image_shape`; device arithmetic in libunidepth_hip.so.

One launch program per (batch, input shape, camera mode): pre-processing (antialiased resize + pad), ConvNeXt-L encoder
(backbones/convnext.py:301-471: depth-wise 7x7 conv, LayerNorm, MFMA GEMMs for stem / down-sampling / MLP, max_stack, class-token
means), V1 decoder (unidepthv1/decoder.py: adapters, fp32 camera head, spherical-harmonics ray embeddings, single-head width-512
attention as GEMM + softmax + GEMM, 8-head flash attention, ConvUpsample stacks, the NystromBlocks as the reference executes them -- a
per-token softmax attention among the h head-vectors, see nystrom_block below), multi-scale merge and back-projection.  Parity: against
oracle/restate_v1.py, pinned to the live reference running on the statement-by-statement restatement of xformers' NystromAttention
(oracle/stubs/xformers; the package itself is un-vendored and absent -- see the oracle header)."""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch

from . import _lib as L
from . import ops
from .module import EngineModule
from .ops import UD_A_CONV3_ZERO, UD_ACT_GELU, UD_ACT_NONE, UD_EPI_F16, UD_EPI_F32, UD_EPI_QKV
from .plan import PlanRecorder
from .weights import _conv3_rows as _conv3_rows_1, _fold_ln, _rup, pack_vit_blocks

CONVNEXT = {"convnext_large": dict(depths=(3, 3, 27, 3), dims=(192, 384, 768, 1536))}     # models/encoder.py:127-136
VIT = {"dinov2_vitl14": dict(D=1024, depth=24, heads=16, output_idx=[5, 12, 18, 24])}        # models/encoder.py:171-186 (hubconf.py:14-17 v1 / vitl14)


# Weight precision.  fp16-rounding the weights is a SYSTEMATIC perturbation of the model: it moves the predicted camera and the
# log-depth of every pixel coherently, where the activations' rounding averages out (tools/v1_precision_study.py: with fp16 x fp16
# operands depth ARel 1.3-1.6e-3 and K error 5e-4 against the fp32 reference; with exact weights 7e-4 and 6e-5).  The reference runs
# UniDepthV1 in fp32 (no autocast, unidepthv1.py:287-373), so every weight goes to the matrix pipes as TWO fp16 terms,
# W = W_hi + W_lo, concatenated along K: [W_hi | W_lo] against A read twice (UdGemm.a_wrap) -- A W_hi^T + A W_lo^T in one fp32
# accumulator, the weights exact to ~22 bits.  UNIDEPTH_V1_WSPLIT=0 keeps single fp16 weights (A/B of the cost).
# Not every GEMM needs it (`tools/v1_precision_study.py placement`, depth ARel on three inputs): all weights split 7.1 / 7.7 / 7.4e-4;
# the ConvNeXt blocks' fc1 (A = the block's LayerNorm output) single fp16, everything else split 7.4 / 8.0 / 7.5e-4 -- within the study's
# noise, a quarter of the encoder's MFMA work saved; the same blocks' fc2 (A = GELU output, every channel's mean positive: a rounding
# error of W shifts an output channel by the same amount at every pixel) 7.8 / 8.5 / 8.1e-4; the depth decoder's LayerNorm-fed GEMMs
# 1.1-1.2e-3: not those.  Default: split everything except the ConvNeXt fc1; UNIDEPTH_V1_WSPLIT=all splits those too.
# UNIDEPTH_V1_WSPLIT: "all" (default since round 4) = every GEMM weight as two fp16 terms; "1" = the round-3 placement (the ConvNeXt blocks'
# fc1 weights single fp16: -6.9 % time, but over 8 checkpoint seeds a global depth shift of up to 8.6e-4 and the one case of the sweep
# left above 1e-3; measured 16 of 16 within the bar, worst 7.9e-4, with them split: DESIGN 10.3b); "0" = single fp16 weights everywhere.
_WSPLIT_ENV = os.environ.get("UNIDEPTH_V1_WSPLIT", "all")
WSPLIT = _WSPLIT_ENV != "0"
WSPLIT_CONVNEXT_FC1 = _WSPLIT_ENV == "all"
# Third product term (round 4): the A operand of the ConvUpsample tails (conv1x1 -> bilinear x2 -> conv3x3, layers/upsample.py:
# 32-36) and of the 3x3 -> 1 output convs (decoder.py:267-271) is carried as TWO fp16 terms [A_hi | A_lo] against [W_hi | W_hi | W_lo].  The
# 8-seed sweep (tests/test_parity_sweep_gpu.py) put the depth error of these nine GEMMs' ACTIVATION rounding at ~1e-3 on some checkpoints
# (tools/r4_v1_seed_study.py: 1.30e-3 -> 8.0e-4 emulated with them exact) -- they sit directly in front of the depth output, where nothing
# averages the noise.  UNIDEPTH_V1_ASPLIT=0: two terms as in round 3 (A/B).
ASPLIT = WSPLIT and os.environ.get("UNIDEPTH_V1_ASPLIT", "1") != "0"


# Round 6: the ConvNeXt blocks' LayerNorm folded into the depth-wise convolution (producer) and fc1 (consumer): UNIDEPTH_V1_DWLN=0 keeps the LayerNorm launches.
DWLN = os.environ.get("UNIDEPTH_V1_DWLN", "1") != "0"


def _split_mode() -> str:
    """The fp16 operand layout in force (module-level switches read once at import): packed weights carry it, plan builders assert it, so weights
    packed under one setting are never multiplied under another (e.g. a [hi | lo] weight against a single-term K)."""
    return f"w{int(WSPLIT)}.fc1{int(WSPLIT_CONVNEXT_FC1)}.a{int(ASPLIT)}"


def _padk16(w: torch.Tensor, split: Optional[bool] = None) -> torch.Tensor:
    """[N, K] fp32 -> fp16 GEMM operand, K zero-padded to a multiple of 64; split: [hi | lo] halves of the padded width each."""
    split = WSPLIT if split is None else split
    n, k = w.shape
    kp = _rup(k, 64)
    hi = w.to(torch.float16)
    out = torch.zeros(n, 2 * kp if split else kp, dtype=torch.float16)
    out[:, :k] = hi
    if split:
        out[:, kp:kp + k] = (w - hi.to(torch.float32)).to(torch.float16)
    return out.contiguous()


def _padk16_3(w: torch.Tensor) -> torch.Tensor:
    """[N, K] fp32 (K % 64 == 0) -> fp16 [N, 3 K] = [W_hi | W_hi | W_lo]: the W operand of a THREE-term product whose A operand is
    [A_hi | A_lo] (2 K wide, wrapping once: UdGemm.a_wrap = 2 K) -- A_hi W_hi + A_lo W_hi + A_hi W_lo."""
    n, k = w.shape
    assert k % 64 == 0, k
    hi = w.to(torch.float16)
    lo = (w - hi.to(torch.float32)).to(torch.float16)
    return torch.cat([hi, hi, lo], dim=1).contiguous()


def _conv3_rows_3(w):
    """[Cout, Cin, 3, 3] -> fp32 [Cout, 9 * 3 * Cin]: per tap [W_hi | W_hi | W_lo] (all exactly representable in fp16) for an image that
    carries [A_hi | A_lo] = 2 Cin channels per pixel (the channel index wraps after 2 Cin: UdGemm.a_wrap)."""
    r = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, -1)
    hi = r.to(torch.float16).to(torch.float32)
    lo = (r - hi).to(torch.float16).to(torch.float32)
    return torch.cat([hi, hi, lo], dim=2).reshape(w.shape[0], -1)


def _wk(Wt: torch.Tensor, K: int, conv_cin: int = 0) -> dict:
    """Descriptor fields of a GEMM whose W operand is a packed weight: K = width of the A operand (conv: 9 * Cin rounded up);
    a split weight is twice as wide and A wraps around (dense: after K columns; conv: after Cin channels of every tap); a THREE-term
    weight ([W_hi | W_hi | W_lo]) is three times as wide and A = [A_hi | A_lo] wraps after 2 K columns / 2 Cin channels."""
    if conv_cin:
        if Wt.shape[1] >= 27 * conv_cin:
            return dict(K=Wt.shape[1], ldw=Wt.shape[1], Cin=3 * conv_cin, a_wrap=2 * conv_cin)
        split = Wt.shape[1] >= 18 * conv_cin
        return dict(K=Wt.shape[1], ldw=Wt.shape[1], Cin=2 * conv_cin if split else conv_cin, **({"a_wrap": conv_cin} if split else {}))
    if Wt.shape[1] == 3 * K:
        return dict(K=3 * K, ldw=3 * K, a_wrap=2 * K)
    if Wt.shape[1] == 2 * K:
        return dict(K=2 * K, ldw=2 * K, a_wrap=K)
    assert Wt.shape[1] == K, (tuple(Wt.shape), K)
    return dict(K=K, ldw=K)


def pack_convnext(config: dict, sd: dict, device) -> dict:
    """Load-time repack of the reference's `pixel_encoder.*` tensors (exact fp32 algebra, then one fp16 rounding of the GEMM operands):
    LayerNorm affines folded into the consuming Linear / down-sampling Conv2d (zero padding 0: exact), block layer-scale `gamma`
    folded into fc2, depth-wise filters tap-major [49][C], stem / down-sampling filters as GEMM rows in im2col column order."""
    a = CONVNEXT[config["model"]["pixel_encoder"]["name"]]
    f = {k: v.detach().to(torch.float32).cpu() for k, v in sd.items() if k.startswith("pixel_encoder.")}
    pe = "pixel_encoder."
    w = {}

    def p16(name, t, split=None):
        w[name] = _padk16(t, split).to(device)

    def p32(name, t):
        w[name] = t.to(torch.float32).contiguous().to(device)

    p16("stem.w", f[pe + "stem.0.weight"].reshape(a["dims"][0], 48)); p32("stem.b", f[pe + "stem.0.bias"])
    p32("stem.g", f[pe + "stem.1.weight"]); p32("stem.beta", f[pe + "stem.1.bias"])
    for s, (dep, d) in enumerate(zip(a["depths"], a["dims"])):
        if s > 0:
            g, b = f[f"{pe}stages.{s}.downsample.0.weight"], f[f"{pe}stages.{s}.downsample.0.bias"]
            wc, bc = f[f"{pe}stages.{s}.downsample.1.weight"], f[f"{pe}stages.{s}.downsample.1.bias"]      # [Cout, Cin, 2, 2]
            p16(f"ds.{s}.w", (wc * g[None, :, None, None]).permute(0, 2, 3, 1).reshape(d, -1))              # columns (ky, kx, cin)
            p32(f"ds.{s}.b", bc + torch.einsum("ocyx,c->o", wc, b))
        for i in range(dep):
            r = f"{pe}stages.{s}.blocks.{i}."
            p32(f"blk.{s}.{i}.dw.w", f[r + "conv_dw.weight"].reshape(d, 49).t()); p32(f"blk.{s}.{i}.dw.b", f[r + "conv_dw.bias"])
            g, b = f[r + "norm.weight"], f[r + "norm.bias"]
            w1, b1 = f[r + "mlp.fc1.weight"], f[r + "mlp.fc1.bias"]
            p16(f"blk.{s}.{i}.fc1.w", w1 * g[None, :], split=WSPLIT_CONVNEXT_FC1); p32(f"blk.{s}.{i}.fc1.b", b1 + w1 @ b)
            # row sums of the fp16 terms the matrix pipe multiplies (hi + lo): the LayerNorm-folded consumer's mean correction (UdGemm.wsum)
            w[f"blk.{s}.{i}.fc1.wsum"] = w[f"blk.{s}.{i}.fc1.w"].float().sum(dim=1).contiguous()
            ls = f[r + "gamma"]
            p16(f"blk.{s}.{i}.fc2.w", f[r + "mlp.fc2.weight"] * ls[:, None]); p32(f"blk.{s}.{i}.fc2.b", f[r + "mlp.fc2.bias"] * ls)
    w["meta.split"] = _split_mode()                    # the operand layout these weights were packed for (checked by the plan builders)
    return w


def _ak(Wt: torch.Tensor, K: int) -> dict:
    """Like _wk for a GEMM whose *A* operand is the packed weight (V^T = W_v X^T): the activations (W operand) wrap around."""
    if Wt.shape[1] == 2 * K:
        return dict(K=2 * K, lda=2 * K, w_wrap=K)
    assert Wt.shape[1] == K, (tuple(Wt.shape), K)
    return dict(K=K, lda=K)


def pack_vit(config: dict, sd: dict, device) -> dict:
    """UniDepthV1 on DINOv2 ViT-L/14: the encoder's GEMM operands through the V2 packer's folds (weights.pack_vit_blocks), stored like every
    other V1 weight (two fp16 terms when WSPLIT); the resampled position embedding / class token stay on the host side per grid."""
    a = VIT[config["model"]["pixel_encoder"]["name"]]
    f = {k: v.detach().to(torch.float32).cpu() for k, v in sd.items() if k.startswith("pixel_encoder.")}
    w = {}

    def put16(name, t, wsum=False):
        w[name] = _padk16(t).to(device)

    def put32(name, t):
        w[name] = t.to(torch.float32).contiguous().to(device)
    pack_vit_blocks(f, a["D"], a["depth"], a["heads"], put16, put32)
    w["host.pos_embed"] = f["pixel_encoder.pos_embed"]
    w["host.cls_token"] = f["pixel_encoder.cls_token"].reshape(-1)
    w["meta.split"] = _split_mode()                    # the operand layout these weights were packed for (checked by the plan builders)
    return w


def vit_pos_embed_v1(pe: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """[1, 1 + M*M, D] -> [1 + h*w, D]: bicubic resample with the SCALE-FACTOR form V1 builds its DINOv2 with (interpolate_offset = 0.1:
    unidepthv1.py:412-421, backbones/dinov2.py:283-296) -- not the output-size form of the V2 models."""
    n = pe.shape[1] - 1
    m = int(math.sqrt(n))
    if h * w == n and h == w:
        return pe[0].contiguous()
    grid = pe[:, 1:].reshape(1, m, m, -1).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, scale_factor=(float(h + 0.1) / m, float(w + 0.1) / m), mode="bicubic", antialias=False)
    assert tuple(grid.shape[-2:]) == (h, w)
    return torch.cat([pe[0, :1], grid.permute(0, 2, 3, 1).reshape(h * w, -1)], 0).contiguous()


def _conv3_rows(w, split: Optional[bool] = None):
    """[Cout, Cin, 3, 3] -> [Cout, 9*Cin], k = (ky*3 + kx)*Cin + ci; split: fp32 [Cout, 9 * 2 * Cin] with the (hi | lo) fp16 terms of every
    tap side by side (both exactly representable in fp16, so the later fp16 cast is exact)."""
    if not (WSPLIT if split is None else split):
        return _conv3_rows_1(w)
    r = w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, -1)
    hi = r.to(torch.float16).to(torch.float32)
    lo = (r - hi).to(torch.float16).to(torch.float32)
    return torch.cat([hi, lo], dim=2).reshape(w.shape[0], -1)


def pack_v1_decoder(config: dict, sd: dict, device) -> dict:
    """Load-time repack of `pixel_decoder.*` (unidepthv1/decoder.py:468-533): LayerNorm affines folded into the consuming Linear, LayerScale /
    CvnxtBlock gammas into the producing one, 1/sqrt(d) of the single-head width-512 attentions into their q projection, conv filters as
    GEMM rows, K padded to 64.  The 4-token camera transformer keeps fp32 weights (fp32 island, as in the V2 engine)."""
    f = {k: v.detach().to(torch.float32).cpu() for k, v in sd.items() if k.startswith("pixel_decoder.")}
    C = config["model"]["pixel_decoder"]["hidden_dim"]
    pd = "pixel_decoder."
    w = {}

    def p16(name, t):
        w[name] = _padk16(t).to(device)

    def p32(name, t):
        w[name] = t.to(torch.float32).contiguous().to(device)

    def lin_ln16(dst, wk, bk, nk):             # LN(nk) -> Linear(wk): fp16 GEMM operand + fp32 bias
        ww, bb = _fold_ln(f[wk + ".weight"], f.get(wk + ".bias"), f[nk + ".weight"], f[nk + ".bias"])
        p16(dst + ".w", ww); p32(dst + ".b", bb)

    def lin_ln32(dst, wk, bk, nk):
        ww, bb = _fold_ln(f[wk + ".weight"], f.get(wk + ".bias"), f[nk + ".weight"], f[nk + ".bias"])
        p32(dst + ".w", ww); p32(dst + ".b", bb)

    for j in range(4):
        a = f"{pd}input_adapter.input_adapters.{j}"
        lin_ln16(f"ad.{j}", a + ".1", None, a + ".0")
        t = f"{pd}token_adapter.input_adapters.{j}"
        lin_ln32(f"tok.{j}", t + ".1", None, t + ".0")
    lv = f[pd + "level_embeds"]
    lv = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(lv, f[pd + "level_embed_layer.0.weight"], f[pd + "level_embed_layer.0.bias"])),
                                    f[pd + "level_embed_layer.2.weight"], f[pd + "level_embed_layer.2.bias"])
    w["host.level_embed"] = torch.nn.functional.layer_norm(lv, (C,), f[pd + "level_embed_layer.3.weight"], f[pd + "level_embed_layer.3.bias"], 1e-5)   # constant of the weights

    def mlp16(dst, src, ls=None):
        lin_ln16(dst + "fc1", src + "proj1", None, src + "norm")
        w2, b2 = f[src + "proj2.weight"], f[src + "proj2.bias"]
        if ls is not None:
            w2, b2 = w2 * ls[:, None], b2 * ls
        p16(dst + "fc2.w", w2); p32(dst + "fc2.b", b2)

    def mlp32(dst, src, ls=None):
        lin_ln32(dst + "fc1", src + "proj1", None, src + "norm")
        w2, b2 = f[src + "proj2.weight"], f[src + "proj2.bias"]
        if ls is not None:
            w2, b2 = w2 * ls[:, None], b2 * ls
        p32(dst + "fc2.w", w2); p32(dst + "fc2.b", b2)

    cl = pd + "camera_layer."
    p32("cam.pos", f[cl + "latents_pos"].reshape(4, C))
    lin_ln32("cam.cls1", cl + "cls_project.1", None, cl + "cls_project.0")
    p32("cam.cls2.w", f[cl + "cls_project.3.weight"]); p32("cam.cls2.b", f[cl + "cls_project.3.bias"])
    mlp16("cam.inf.", cl + "in_features.")
    a = cl + "aggregate."
    lin_ln32("cam.agg.q", a + "q", None, a + "norm_attnx")
    lin_ln16("cam.agg.kv", a + "kv", None, a + "norm_attnctx")
    p32("cam.agg.out.w", f[a + "out.weight"] * f[a + "ls1.gamma"][:, None]); p32("cam.agg.out.b", f[a + "out.bias"] * f[a + "ls1.gamma"])
    mlp32("cam.agg.", a + "mlp.", f[a + "ls2.gamma"])
    for i in range(2):
        a = f"{cl}layers.{i}."
        lin_ln32(f"cam.l{i}.q", a + "q", None, a + "norm_attnx")
        lin_ln32(f"cam.l{i}.kv", a + "kv", None, a + "norm_attnctx")
        p32(f"cam.l{i}.out.w", f[a + "out.weight"] * f[a + "ls1.gamma"][:, None]); p32(f"cam.l{i}.out.b", f[a + "out.bias"] * f[a + "ls1.gamma"])
        mlp32(f"cam.l{i}.", a + "mlp.", f[a + "ls2.gamma"])
    mlp32("cam.out.", cl + "out.")

    dl = pd + "depth_layer."
    for nm in ("project_rays16", "project_rays8", "project_rays4"):
        mlp16(f"{nm}.", f"{dl}{nm}.")                                  # K: 81 -> 128, 324 -> 384 (zero padded)
    wc = f[dl + "features_channel_cat.weight"]
    for j in range(4):
        p16(f"fcat.{j}.w", wc[:, j * C:(j + 1) * C])
    p32("fcat.0.b", f[dl + "features_channel_cat.bias"])
    mlp16("tolat.", dl + "to_latents.")

    def big_attn(dst, src):                    # single head of width C: q pre-scaled by C^-1/2; K and V projections separate (V^T is produced by a GEMM)
        sc = C ** -0.5
        wq, bq = _fold_ln(f[src + "q.weight"], f[src + "q.bias"], f[src + "norm_attnx.weight"], f[src + "norm_attnx.bias"])
        p16(dst + "q.w", wq * sc); p32(dst + "q.b", bq * sc)
        wkv, bkv = _fold_ln(f[src + "kv.weight"], f[src + "kv.bias"], f[src + "norm_attnctx.weight"], f[src + "norm_attnctx.bias"])
        p16(dst + "k.w", wkv[:C]); p32(dst + "k.b", bkv[:C])
        p16(dst + "v.w", wkv[C:]); p32(dst + "v.b", bkv[C:])
        p16(dst + "out.w", f[src + "out.weight"] * f[src + "ls1.gamma"][:, None]); p32(dst + "out.b", f[src + "out.bias"] * f[src + "ls1.gamma"])
        mlp16(dst, src + "mlp.", f[src + "ls2.gamma"])

    big_attn("agg16.", dl + "aggregate_16.")
    big_attn("pcam.", dl + "prompt_camera.")
    depths = list(config["model"]["pixel_decoder"]["depths"])
    for i in range(depths[0]):
        src, dst = f"{dl}layers_16.{i}.", f"l16.{i}."
        lin_ln16(dst + "q", src + "q", None, src + "norm_attnx")
        lin_ln16(dst + "kv", src + "kv", None, src + "norm_attnctx")
        p16(dst + "out.w", f[src + "out.weight"] * f[src + "ls1.gamma"][:, None]); p32(dst + "out.b", f[src + "out.bias"] * f[src + "ls1.gamma"])
        mlp16(dst, src + "mlp.", f[src + "ls2.gamma"])
    for nm, d, n in (("layers_8", C // 2, depths[1]), ("layers_4", C // 4, depths[2])):
        for i in range(n):
            src, dst = f"{dl}{nm}.{i}.", f"{nm}.{i}."
            lin_ln16(dst + "q", src + "q", None, src + "norm_attnx")
            wkv, bkv = _fold_ln(f[src + "kv.weight"], f[src + "kv.bias"], f[src + "norm_attnctx.weight"], f[src + "norm_attnctx.bias"])
            p16(dst + "kv.w", wkv); p32(dst + "kv.b", bkv)       # one [K | V] GEMM
            p16(dst + "out.w", f[src + "out.weight"] * f[src + "ls1.gamma"][:, None]); p32(dst + "out.b", f[src + "out.bias"] * f[src + "ls1.gamma"])
            mlp16(dst, src + "mlp.", f[src + "ls2.gamma"])
    for nm, d in (("up8", C), ("up4", C // 2), ("up2", C // 4)):
        for c in range(2):
            src, dst = f"{dl}{nm}.convs.{c}.", f"{nm}.{c}."
            p32(dst + "dw.w", f[src + "dwconv.weight"].reshape(d, 49).t()); p32(dst + "dw.b", f[src + "dwconv.bias"])
            w1, b1 = _fold_ln(f[src + "pwconv1.weight"], f[src + "pwconv1.bias"], f[src + "norm.weight"], f[src + "norm.bias"])
            p16(dst + "fc1.w", w1); p32(dst + "fc1.b", b1)
            g = f[src + "gamma"]
            p16(dst + "fc2.w", f[src + "pwconv2.weight"] * g[:, None]); p32(dst + "fc2.b", f[src + "pwconv2.bias"] * g)
        if ASPLIT:
            w[f"{nm}.up0.w"] = _padk16_3(f[f"{dl}{nm}.up.0.weight"].reshape(d // 2, d)).to(device)
            w[f"{nm}.up2.w"] = _padk16(_conv3_rows_3(f[f"{dl}{nm}.up.2.weight"]), split=False).to(device)
        else:
            p16(f"{nm}.up0.w", f[f"{dl}{nm}.up.0.weight"].reshape(d // 2, d))
            w[f"{nm}.up2.w"] = _padk16(_conv3_rows(f[f"{dl}{nm}.up.2.weight"]), split=False).to(device)
        p32(f"{nm}.up0.b", f[f"{dl}{nm}.up.0.bias"]); p32(f"{nm}.up2.b", f[f"{dl}{nm}.up.2.bias"])
    for nm, d in (("out8", C // 2), ("out4", C // 4), ("out2", C // 8)):
        # one output channel: a VALU stencil over the fp32 map (UD_V1_OUT_CONV3), weights [tap = ky * 3 + kx, c] in fp32, the bias on the host
        p32(f"{nm}.cw", f[f"{dl}{nm}.weight"][0].permute(1, 2, 0).reshape(9, d))
        w[f"host.{nm}.bias"] = float(f[f"{dl}{nm}.bias"][0])
    w["meta.split"] = _split_mode()                    # the operand layout these weights were packed for (checked by the plan builders)
    return w


class _EncPlan(PlanRecorder):
    """Device buffers + launch program of the ConvNeXt encoder for one (batch, network image shape)."""

    def __init__(self, model: "UniDepthV1", B: int, Hn: int, Wn: int, P: Optional[ops.Program] = None, img: Optional[torch.Tensor] = None):
        super().__init__(model._w, model.device, P)
        w, z, P = self.weights, self.z, self.prog
        f32 = torch.float32
        self.B = B
        self.img = z(B, 3, Hn, Wn, dtype=f32) if img is None else img
        H, W = Hn // 4, Wn // 4
        dims, depths = model._arch["dims"], model._arch["depths"]
        rows = B * H * W
        patches = z(rows, 64)
        P.patchify4(self.img, patches, B, Hn, Wn, 64)
        x0 = z(rows, dims[0], dtype=f32)
        P.gemm(A=patches, W=w["stem.w"], bias=w["stem.b"], out=x0, M=rows, N=dims[0], lda=64, ldc=dims[0], epi=UD_EPI_F32, tag="stem", **_wk(w["stem.w"], 64))
        x = z(rows, dims[0], dtype=f32)
        P.layernorm(x=x0, y=x, rows=rows, D=dims[0], ldx=dims[0], ldy=dims[0], eps=1e-6, rows_per_img=rows, in_rows_per_img=rows,
                    out_rows_per_img=rows, out_f32=1, gamma=w["stem.g"], beta=w["stem.beta"])
        self.tap("stem", lambda x=x, H=H, W=W, C=dims[0]: x.view(B, H, W, C).permute(0, 3, 1, 2).clone())
        self.shapes, self.stage_max, self.cls, self.dwln = [], [], [], []
        nblk = sum(depths)
        for s, (dep, C) in enumerate(zip(depths, dims)):
            if s > 0:
                Cp = dims[s - 1]
                Ho, Wo = H // 2, W // 2
                rows = B * Ho * Wo
                col = z(rows, 4 * Cp)
                P.layernorm_patchify2(x, col, B, H, W, Cp, 4 * Cp, 1e-6)
                xn = z(rows, C, dtype=f32)
                P.gemm(A=col, W=w[f"ds.{s}.w"], bias=w[f"ds.{s}.b"], out=xn, M=rows, N=C, lda=4 * Cp, ldc=C, epi=UD_EPI_F32,
                       tag=f"downsample.{s}", **_wk(w[f"ds.{s}.w"], 4 * Cp))
                x, H, W = xn, Ho, Wo
            self._stage(s, dep, x, H, W, C, first_blk=sum(depths[:s]), cls_from=nblk - 4)

    def _stage(self, s, dep, x, H, W, C, first_blk, cls_from):
        """The blocks of stage s on the fp32 map x [B*H*W, C] (convnext.py:203-226), the stage's running maximum and the class tokens."""
        w, z, P, B = self.weights, self.z, self.prog, self.B
        f32 = torch.float32
        rows = B * H * W
        xh = z(rows, C)
        hid = z(rows, 4 * C)
        smax = z(rows, C, dtype=f32)
        # Round 6: the block's LayerNorm (convnext.py:215-216) folded into its neighbours -- the depth-wise convolution writes its output as RAW fp16
        # plus per-pixel partial sums (UdDwConv7.y16 / stats_out), the last channel block of a pixel tile reduces them to (rstd, -mean rstd)
        # (stats_final), fc1 normalises in its epilogue
        # (UdGemm.row_stats_in): no LayerNorm launch, no fp32 round trip of the map.  Where the large-tile kernel takes fc1 and C / 64 <= 16 (stages
        # 0-2 of ConvNeXt-L; stage 3 has 24 slabs) and UNIDEPTH_V1_DWLN != 0.
        fc1 = dict(out=hid, M=rows, N=4 * C, lda=C, ldc=4 * C, epi=UD_EPI_F16, act=UD_ACT_GELU, **_wk(w[f"blk.{s}.0.fc1.w"], C))
        rstats = z(rows, 2, dtype=f32)
        fold = (DWLN and C % 64 == 0 and C // 64 <= 16 and f"blk.{s}.0.fc1.wsum" in w and
                (ops.gemm_pick(A=xh, W=w[f"blk.{s}.0.fc1.w"], bias=w[f"blk.{s}.0.fc1.b"], row_stats_in=rstats, wsum=w[f"blk.{s}.0.fc1.wsum"], **fc1) & L.UD_PICK_SCHEDULE) in L.UD_PICK_LARGE_TILE)
        self.dwln.append(bool(fold))
        dw = dict(B=B, H=H, W=W, C=C, ldx=C, ldy=C, tag=f"dwconv.s{s}")
        if fold:
            rpart = z(rows, C // 64, 2, dtype=f32)
            tk = torch.zeros(B * -(-H // 8) * -(-W // 16) + 8, dtype=torch.int32, device=self.dev)     # one ticket per 8 x 16 pixel tile (self-resetting)
            dw.update(y16=xh, ldy16=C, stats_out=rpart, stats_final=rstats, stats_ticket=tk, ln_eps=1e-6)
            fc1.update(row_stats_in=rstats, ln_slabs=C // 64, ln_D=C, ln_eps=1e-6)
        else:
            y = z(rows, C, dtype=f32)
            dw.update(y=y)
        for i in range(dep):
            blk = first_blk + i
            P.dwconv7(x=x, w=w[f"blk.{s}.{i}.dw.w"], bias=w[f"blk.{s}.{i}.dw.b"], **dw)
            if not fold:
                P.layernorm(x=y, y=xh, rows=rows, D=C, ldx=C, ldy=C, eps=1e-6, rows_per_img=rows, in_rows_per_img=rows, out_rows_per_img=rows)
            P.gemm(A=xh, W=w[f"blk.{s}.{i}.fc1.w"], bias=w[f"blk.{s}.{i}.fc1.b"], tag=f"enc.fc1.s{s}",
                   **({"wsum": w[f"blk.{s}.{i}.fc1.wsum"]} if fold else {}), **fc1)
            # the stage's running maximum over its block outputs (max_stack) is taken in this epilogue, where the value is produced
            P.gemm(A=hid, W=w[f"blk.{s}.{i}.fc2.w"], bias=w[f"blk.{s}.{i}.fc2.b"], out=x, M=rows, N=C, lda=4 * C, ldc=C,
                   epi=UD_EPI_F32, accumulate=1, tag=f"enc.fc2.s{s}", max_out=smax, max_init=int(i == 0), **_wk(w[f"blk.{s}.{i}.fc2.w"], 4 * C))
            if blk >= cls_from:                        # the decoder reads the class tokens of the LAST four blocks (decoder.py:375-377)
                cbuf = z(B, C, dtype=f32)
                P.spatial_mean(x, cbuf, B, H * W, C, C)
                self.cls.append(cbuf)
            self.tap(f"block{blk}", lambda x=x, H=H, W=W, C=C: x.view(B, H, W, C).clone())
        self.shapes.append((H, W, C))
        self.stage_max.append(smax)


class _EncPlanViT(PlanRecorder):
    """DINOv2 ViT-L/14 as UniDepthV1 runs it (backbones/dinov2.py:306-347 with use_norm False: no final LayerNorm, every block is an output;
    unidepthv1.py:322-328 adds each block's class token to its patch tokens): the V2 engine's block program (plan.PlanRecorder.vit_embed /
    vit_blocks: LayerNorm statistics kernel, fused qkv / attention / proj / fc1 + GELU / fc2 GEMMs) + after every block the running max of its
    level and, for the last four blocks, the class token (UD_V1_VIT_TAP).  Same attributes as _EncPlan: shapes, stage_max, cls."""

    def __init__(self, model: "UniDepthV1", B: int, Hn: int, Wn: int, P: Optional[ops.Program] = None, img: Optional[torch.Tensor] = None):
        from . import _lib as L
        super().__init__(model._w, model.device, P)
        w, z, a = self.weights, self.z, model._arch
        D, depth, ends = a["D"], a["depth"], a["output_idx"]
        f32 = torch.float32
        assert Hn % 14 == 0 and Wn % 14 == 0, "UniDepthV1 / ViT: the network image must be a multiple of the patch size"
        self.B = B
        self.img = z(B, 3, Hn, Wn, dtype=f32) if img is None else img
        h, wg = Hn // 14, Wn // 14
        hw = h * wg
        N = hw + 1
        Np = _rup(N, 16)
        patches = z(B * hw, 640)
        self.prog.preprocess(rgb=self.img, patches=patches, B=B, H=Hn, W=Wn, pad_l=0, pad_t=0, Hp=Hn, Wp=Wn, Hn=Hn, Wn=Wn, ldp=640, is_u8=0, normalize=0,
                             mean=(0.0, 0.0, 0.0), inv_std=(1.0, 1.0, 1.0))
        pos = vit_pos_embed_v1(w["host.pos_embed"], h, wg).to(self.dev)
        cls_row = (w["host.cls_token"] + pos[0].cpu()).to(self.dev)
        x = self.vit_embed(patches, pos, cls_row, B, hw, D, tag="vit.patch")
        self.stage_max = [z(B * hw, D, dtype=f32) for _ in range(4)]
        self.cls = []

        def hook(i, where, x, qk, vt):
            if where != "end":
                return
            lvl = sum(i >= e for e in ends)                 # the level whose block range [ends[lvl - 1], ends[lvl]) holds block i
            first = i == (0 if lvl == 0 else ends[lvl - 1])
            cbuf = None
            if i >= depth - 4:                              # class tokens of the LAST four blocks (decoder.py:375-377), block order
                cbuf = z(B, D, dtype=f32)
                self.cls.append(cbuf)
            self.prog.v1(L.UD_V1_VIT_TAP, a=x, out=self.stage_max[lvl], out2=cbuf, i=(B, Np, hw, D, int(first)), tag="vit_tap")
            self.tap(f"block{i}", lambda x=x: x.view(B, Np, D)[:, :N].clone())

        self.vit_blocks(x, B, hw, a, prefix="vit.", hook=hook)
        self.shapes = [(h, wg, D)] * 4
        self.keep = [x, patches, pos, cls_row]


class UniDepthV1(EngineModule):
    """Engine counterpart of the reference's UniDepthV1 (unidepthv1.py:97-103: nn.Module + PyTorchModelHubMixin).  See the module docstring for
    what runs today; the nn.Module surface is unidepth_amd/module.py."""

    def __init__(self, config: dict, eps: float = 1e-6, **kwargs):
        super().__init__()
        self.config = config
        name = config["model"]["pixel_encoder"]["name"]
        if name in VIT:                              # DINOv2 ViT-L/14 (config_v1_vitl14): levels = block ranges ending at output_idx
            self._arch = dict(VIT[name], kind="vit")
            self._arch["output_idx"] = list(config["model"]["pixel_encoder"].get("output_idx", VIT[name]["output_idx"]))
            oi = self._arch["output_idx"]
            if len(oi) != 4 or oi != sorted(oi) or oi[-1] != self._arch["depth"] or oi[0] < 1:
                raise NotImplementedError(f"UniDepthV1 / ViT output_idx {oi}: four increasing block counts ending at {self._arch['depth']} expected")
        elif name in CONVNEXT:
            self._arch = dict(CONVNEXT[name], kind="convnext")
            self._arch["output_idx"] = list(config["model"]["pixel_encoder"].get("output_idx", [3, 6, 33, 36]))
            ends = [sum(self._arch["depths"][:i + 1]) for i in range(4)]
            if self._arch["output_idx"] != ends:
                # the encoder program takes the element-wise max over WHOLE stages and the class tokens of the last four blocks
                raise NotImplementedError(f"UniDepthV1 pixel_encoder.output_idx {self._arch['output_idx']}: only the stage ends {ends} are implemented")
        else:
            raise NotImplementedError(f"UniDepthV1 pixel_encoder {name!r}: the ConvNeXt-L (config_v1_cnvnxtl) and DINOv2 ViT-L/14 (config_v1_vitl14) "
                                      "backbones are implemented on this engine")
        self.image_shape = list(config["data"]["image_shape"])                         # unidepthv1.py:444
        self.max_plans = max(1, int(os.environ.get("UNIDEPTH_MAX_PLANS", "4")))

    def _pack(self):
        w = (pack_vit if self._arch["kind"] == "vit" else pack_convnext)(self.config, self._sd, self._device)
        if any(k.startswith("pixel_decoder.") for k in self._sd):
            w.update(pack_v1_decoder(self.config, self._sd, self._device))
        return w

    def _enc_plan(self, B, Hn, Wn) -> _EncPlan:
        return self._cached_plan(("enc", B, Hn, Wn), lambda: (_EncPlanViT if self._arch["kind"] == "vit" else _EncPlan)(self, B, Hn, Wn))

    # ---- encoder seam (backbones/convnext.py:447-458) ----
    @property
    def embed_dim(self):
        return self._arch["D"] if self._arch["kind"] == "vit" else 192

    @property
    def patch_size(self):                                                             # unidepthv1.py:427-429: 14 for DINO encoders, else 16
        return 14 if self._arch["kind"] == "vit" else 16

    @property
    def embed_dims(self):
        if self._arch["kind"] == "vit":
            return [self._arch["D"]] * self._arch["depth"]
        return [d for dep, d in zip(self._arch["depths"], self._arch["dims"]) for _ in range(dep)]

    @property
    def depths(self):
        return list(self._arch["output_idx"])

    @torch.no_grad()
    def pixel_encoder(self, image: torch.Tensor, keep_all: bool = True):
        """image [B,3,H,W] (normalised network image) -> (outs, cls_tokens) like ConvNeXt.forward: 36 block outputs [B,h,w,C] and their
        spatial means [B,1,C].  keep_all=False skips copying the 32 intermediate block outputs out of the reused stream buffers and
        returns None for them (the decoder only reads stage-wise maxima and the last four class tokens: see stage_features())."""
        self._ensure_packed()
        B, _, Hn, Wn = image.shape
        with torch.cuda.device(self._device):
            plan = self._enc_plan(B, Hn, Wn)
            plan.img.copy_(image.to(self._device, torch.float32), non_blocking=True)
            vit = self._arch["kind"] == "vit"
            n = self._arch["depth"] if vit else sum(self._arch["depths"])
            outs: List[Optional[torch.Tensor]] = [None] * n
            if vit:                                        # DINOv2 wrapper (backbones/dinov2.py:324-347): patch tokens [B,h,w,D] and class tokens [B,1,D] per block
                h, w_, D = plan.shapes[0]
                cls_v: List[Optional[torch.Tensor]] = [None] * n
                pos = 0
                for name, at, fn in plan.tap_points:
                    plan.prog.run(pos, at)
                    pos = at
                    if keep_all or int(name[5:]) >= n - 4:
                        xb = fn()
                        outs[int(name[5:])] = xb[:, 1:].reshape(B, h, w_, D).contiguous() if keep_all else None
                        cls_v[int(name[5:])] = xb[:, :1].contiguous()
                plan.prog.run(pos, len(plan.prog))
                return outs, cls_v
            if keep_all:
                pos = 0
                for name, at, fn in plan.tap_points:
                    if not name.startswith("block"):
                        continue
                    plan.prog.run(pos, at)
                    pos = at
                    outs[int(name[5:])] = fn()
                plan.prog.run(pos, len(plan.prog))
            else:
                plan.prog.run()
            cls: List[Optional[torch.Tensor]] = [None] * n
            for j, cb in enumerate(plan.cls):
                cls[n - 4 + j] = cb.clone().unsqueeze(1)
            if keep_all:                                   # class tokens of the other blocks: same reduction kernel on the copies
                for i, o in enumerate(outs):
                    if cls[i] is None and o is not None:
                        t = torch.empty(B, o.shape[-1], dtype=torch.float32, device=self._device)
                        ops.check(ops.lib.ud_spatial_mean_f32(o.data_ptr(), t.data_ptr(), B, o.shape[1] * o.shape[2], o.shape[3], o.shape[3],
                                                              ops.cur_stream()), "ud_spatial_mean_f32")
                        cls[i] = t.unsqueeze(1)
        return outs, cls

    @torch.no_grad()
    def stage_features(self, image: torch.Tensor):
        """What the V1 decoder consumes (decoder.py:366-377): per stage the element-wise max over its block outputs [B,h,w,C], and the
        class tokens of the last four blocks, deepest first."""
        self._ensure_packed()
        B, _, Hn, Wn = image.shape
        with torch.cuda.device(self._device):
            plan = self._enc_plan(B, Hn, Wn)
            plan.img.copy_(image.to(self._device, torch.float32), non_blocking=True)
            plan.prog.run()
            feats = [m.view(B, h, w, c).clone() for m, (h, w, c) in zip(plan.stage_max, plan.shapes)]
            cls = [plan.cls[-i - 1].clone().unsqueeze(1) for i in range(4)]
        return feats, cls

    def _full_plan(self, *sig) -> "_FullPlan":
        return self._cached_plan(("full",) + tuple(sig), lambda: _FullPlan(self, *sig))

    @torch.no_grad()
    def infer(self, rgbs: torch.Tensor, intrinsics=None, skip_camera: bool = False):
        """Same contract as the reference (unidepthv1.py:288-373): rgbs uint8 / float [3,H,W] or [B,3,H,W], optional pinhole intrinsics
        [3,3] / [B,3,3] of the INPUT image, skip_camera (use the given camera instead of running the camera head)
        -> {"intrinsics" [B,3,3], "points" [B,3,H,W], "depth" [B,1,H,W]} at the input resolution."""
        self._ensure_packed()
        if rgbs.ndim == 3:
            rgbs = rgbs.unsqueeze(0)
        if intrinsics is not None and intrinsics.ndim == 2:
            intrinsics = intrinsics.unsqueeze(0)
        B, _, H, W = rgbs.shape
        is_u8 = rgbs.dtype == torch.uint8
        if is_u8:
            div255, normalize = True, True
        else:                                   # the reference inspects the value range of float inputs (unidepthv1.py:305-313)
            mn, mx = float(rgbs.min()), float(rgbs.max())
            div255 = mx > 5
            if div255:
                mn, mx = mn / 255.0, mx / 255.0
            normalize = mn >= 0.0 and mx <= 1.0
        n_gt = 0 if intrinsics is None else int(intrinsics.shape[0])
        assert n_gt in (0, 1, B), f"intrinsics batch {n_gt} does not match the image batch {B}"
        skip = bool(skip_camera and intrinsics is not None)
        with torch.cuda.device(self._device):
            plan = self._full_plan(B, H, W, is_u8, div255, normalize, n_gt, skip)
            plan.rgb.copy_(rgbs if is_u8 else rgbs.float(), non_blocking=True)
            pl, pr, pt, pb = plan.pads
            gtK = None
            if intrinsics is not None:
                gtK = intrinsics.detach().float().cpu().clone()                 # _preprocess (unidepthv1.py:57-63)
                gtK[:, 0, 0] *= plan.ratio; gtK[:, 1, 1] *= plan.ratio
                gtK[:, 0, 2] = gtK[:, 0, 2] * plan.ratio + pl
                gtK[:, 1, 2] = gtK[:, 1, 2] * plan.ratio + pt
                kinv = torch.zeros(n_gt, 3, 3)
                kinv[:, 0, 0], kinv[:, 1, 1], kinv[:, 2, 2] = 1.0 / gtK[:, 0, 0], 1.0 / gtK[:, 1, 1], 1.0
                kinv[:, 0, 2], kinv[:, 1, 2] = -gtK[:, 0, 2] / gtK[:, 0, 0], -gtK[:, 1, 2] / gtK[:, 1, 1]
                plan.Kinv_gt.copy_(kinv.reshape(n_gt, 9))
            plan.prog.run()
            dev = self._device
            points = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
            depth = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
            if gtK is None:
                Kret = plan.Kpost.view(B, 3, 3).clone()
                Kuse, nK = plan.Kpost, B
            elif skip:                          # the "predicted" matrix IS the GT tensor, rescaled in place by _postprocess (unidepthv1.py:343-358)
                Kp = gtK.clone()
                Kp[:, 0, 0] /= plan.ratio; Kp[:, 1, 1] /= plan.ratio
                Kp[:, 0, 2] = (Kp[:, 0, 2] - pl) / plan.ratio
                Kp[:, 1, 2] = (Kp[:, 1, 2] - pt) / plan.ratio
                Kuse = Kp.reshape(n_gt, 9).to(dev)
                Kret, nK = Kuse.view(n_gt, 3, 3).expand(B, 3, 3).clone(), n_gt
            else:                               # reference quirk: back-projection with the NETWORK-resolution GT matrix on the input pixel grid (:358)
                Kret = plan.Kpost.view(B, 3, 3).clone()
                Kuse, nK = gtK.reshape(n_gt, 9).to(dev), n_gt
            ops.v1_op(L.UD_V1_POINTS, a=plan.zout, b=Kuse, out=points, out2=depth, i=(B, H, W, 4, nK))
        return {"intrinsics": Kret, "points": points, "depth": depth}

    __call__ = infer

    def forward_test(self, inputs, image_metas=None, **kwargs):
        """The reference's validation forward (unidepthv1.py forward_test).  Not available: UniDepthV1 has no network-resolution plan
        here (its launch program starts from the input image); UniDepthV2.forward_test is the implemented one."""
        raise NotImplementedError("UniDepthV1.forward_test: not implemented -- UniDepthV1 has no network-resolution plan on this engine; "
                                  "use infer() per image, or UniDepthV2.forward_test")

    @torch.no_grad()
    def infer_with_taps(self, rgbs: torch.Tensor, intrinsics=None, skip_camera: bool = False):
        """infer() + the decoder's intermediate tensors (segmented replay of the launch program; parity tooling)."""
        out = self.infer(rgbs, intrinsics, skip_camera)             # builds / refreshes the plan and its inputs
        plan = next(reversed(self._plans.values()))
        taps, pos = {}, 0
        with torch.cuda.device(self._device):
            for name, at, fn in sorted(plan.tap_points, key=lambda t: t[1]):
                if at > pos:
                    plan.prog.run(pos, at)
                    pos = at
                taps[name] = fn()
            plan.prog.run(pos, len(plan.prog))
        return out, taps

# =====================================================================================================================
# Full infer() plan: pre-processing + encoder + decoder + post-processing
# =====================================================================================================================
def v1_shapes(image_shape, network_shape):
    """unidepthv1.py:38-47 _shapes + :29-35 _paddings: ((h, w) after the aspect-preserving resize, ratio, (pad_l, pad_r, pad_t, pad_b))."""
    h, w = image_shape
    if network_shape[1] / network_shape[0] > w / h:
        ratio = network_shape[0] / h
    else:
        ratio = network_shape[1] / w
    nh, nw = math.ceil(h * ratio - 0.5), math.ceil(w * ratio - 0.5)
    Hn, Wn = network_shape
    pt, pb = (Hn - nh) // 2, Hn - nh - (Hn - nh) // 2
    pl, pr = (Wn - nw) // 2, Wn - nw - (Wn - nw) // 2
    return (nh, nw), ratio, (pl, pr, pt, pb)


def pos_embed_sine(h: int, w: int, num_pos_feats: int, temperature: float = 10000.0) -> torch.Tensor:
    """PositionEmbeddingSine(num_pos_feats, normalize=True) of an unmasked h x w grid (layers/positional_encoding.py:14-57) -> [h*w, 2*npf].
    A constant of the grid shape, computed once per plan on the host (like the V2 engine's resampled position embedding)."""
    eps, scale = 1e-6, 2 * math.pi
    yy = torch.arange(1, h + 1, dtype=torch.float32)[:, None].expand(h, w) / (h + eps) * scale
    xx = torch.arange(1, w + 1, dtype=torch.float32)[None, :].expand(h, w) / (w + eps) * scale
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    px, py = xx[:, :, None] / dim_t, yy[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).reshape(h * w, -1)


class _FullPlan(PlanRecorder):
    """One launch program for infer(): unidepthv1.py:288-373 -> decoder.py:364-463 (Decoder.forward), :39-111 (CameraHead), :231-330
    (DepthHead.forward).  Token streams are fp32 [B*n, C]; MFMA operands fp16; the 4-token camera transformer runs in fp32."""

    def __init__(self, model: "UniDepthV1", B: int, H: int, W: int, is_u8: bool, div255: bool, normalize: bool, n_gt: int, skip_camera: bool):
        super().__init__(model._w, model.device)
        w = self.weights
        assert w.get("meta.split") == _split_mode(), f"weights packed for operand layout {w.get('meta.split')!r}, plans built for {_split_mode()!r}"
        self.C = model.config["model"]["pixel_decoder"]["hidden_dim"]
        self.heads = model.config["model"]["num_heads"]
        dec_depths = list(model.config["model"]["pixel_decoder"]["depths"])
        Hn, Wn = model.image_shape
        self.B, self.H, self.W, self.Hn, self.Wn = B, H, W, Hn, Wn
        self.shape_in, self.ratio, self.pads = v1_shapes((H, W), (Hn, Wn))
        self.n_gt, self.skip = n_gt, skip_camera
        self.nb = n_gt if n_gt else B      # batch of the ray tensors (one GT camera broadcasts)
        self.zeros = self.z(256)
        enc = self._preprocess_and_encode(model, is_u8, div255, normalize)
        feat, feat16, pos_lvl = self._adapters(enc)
        self._camera_head(enc, feat, pos_lvl)
        e16, e8, e4 = self._rays_and_embeddings()
        lat = self._latents(feat16)
        self._layers_16(lat, feat, pos_lvl, e16, dec_depths[0])
        outs = self._pyramid(lat, (e16, e8, e4), dec_depths)
        self._merge_and_postprocess(outs)

    # ---------------- recording helpers
    def _ln(self, src, dst, rows, D, eps=1e-5, **kw):
        self.prog.layernorm(x=src, y=dst, rows=rows, D=D, ldx=D, ldy=D, eps=eps, **dict(dict(rows_per_img=rows, in_rows_per_img=rows, out_rows_per_img=rows), **kw))

    def _wgemm(self, A, Wn_, out, M, N, K, bias=True, **kw):
        """GEMM on the packed weight `Wn_` (+ its bias), K / ldw / a_wrap from the weight's operand layout (_wk)."""
        w = self.weights
        self.prog.gemm(A=A, W=w[Wn_ + ".w"], out=out, M=M, N=N, lda=kw.pop("lda", K), ldc=kw.pop("ldc", N),
                       **({"bias": w[Wn_ + ".b"]} if bias else {}), tag=kw.pop("tag", "v1." + Wn_), **_wk(w[Wn_ + ".w"], K), **kw)

    def _mlp(self, stream, pre, rows, D, accumulate=1, out=None, n_out=None):
        """x (+)= fc2(GELU(fc1(LN(x))))  (layers/mlp.py:27-35; LayerScale folded into fc2)."""
        nh = self.weights[pre + "fc1.w"].shape[0]
        xn = self.z(rows, D)
        hid = self.z(rows, _rup(nh, 64))
        self._ln(stream, xn, rows, D)
        self._wgemm(xn, pre + "fc1", hid, rows, nh, D, epi=UD_EPI_F16, act=UD_ACT_GELU, ldc=_rup(nh, 64))
        n_out = D if n_out is None else n_out
        self._wgemm(hid, pre + "fc2", stream if out is None else out, rows, n_out, _rup(nh, 64), epi=UD_EPI_F32, accumulate=accumulate)

    # ---------------- pre-processing + encoder
    def _preprocess_and_encode(self, model, is_u8, div255, normalize):
        B, H, W, Hn, Wn = self.B, self.H, self.W, self.Hn, self.Wn
        (h_in, w_in), (pl, pr, pt, pb) = self.shape_in, self.pads
        self.rgb = torch.zeros(B, 3, H, W, dtype=torch.uint8 if is_u8 else torch.float32, device=self.dev)
        img = self.z(B, 3, Hn, Wn, dtype=torch.float32)
        self.prog.v1(L.UD_V1_PREPROCESS, a=self.rgb, out=img, i=(B, H, W, h_in, w_in, Hn, Wn, pl, pt, int(is_u8), int(div255), int(normalize)), tag="preprocess")
        enc = (_EncPlanViT if model._arch["kind"] == "vit" else _EncPlan)(model, B, Hn, Wn, P=self.prog, img=img)
        self.enc = enc
        self.dec_first = len(self.prog)
        # level shapes as the reference derives them (decoder.py:380-392): sorted (short, long) sides, common = second smallest level
        lv = [tuple(sorted((hh, ww))) for hh, ww, _ in enc.shapes]
        level_shapes = sorted(set(lv))[::-1]
        if len(level_shapes) == 1:                  # ViT: one resolution for all four levels (decoder.py:391-392)
            level_shapes = level_shapes * 4
        assert len(level_shapes) == 4, "UniDepthV1 decoder: the encoder levels must have four distinct resolutions, or one"
        self.h, self.wd = level_shapes[-2]
        self.hw = self.h * self.wd
        return enc

    # ---------------- encoder features -> common resolution -> adapters (decoder.py:394-411, :21-36)
    def _adapters(self, enc):
        z, B, C, h, wd, hw = self.z, self.B, self.C, self.h, self.wd, self.hw
        f32 = torch.float32
        Mt = B * hw
        feat = [z(Mt, C, dtype=f32) for _ in range(4)]           # adapted features, level-major like the reference's list
        feat16 = [z(Mt, C) for _ in range(4)]
        for j, (hh, ww, Cj) in enumerate(enc.shapes):
            src = enc.stage_max[j]
            if (hh, ww) != (h, wd):
                rs = z(Mt, Cj, dtype=f32)
                self.prog.v1(L.UD_V1_RESIZE_AA, a=src, out=rs, i=(B, hh, ww, h, wd, Cj, Cj, Cj, 0, 0, hh, ww), tag="resize_aa")
                src = rs
            xn = z(Mt, Cj)
            self._ln(src, xn, Mt, Cj)
            self._wgemm(xn, f"ad.{j}", feat[j], Mt, C, Cj, epi=UD_EPI_F32, act=UD_ACT_GELU, out2=feat16[j], ldc2=C)
        self.tap("features", lambda: [t.view(B, hw, C).clone() for t in feat])
        pos = pos_embed_sine(h, wd, C // 2)                                   # [hw, C]
        pos_lvl = (pos[None] + self.weights["host.level_embed"][:, None, :]).reshape(4 * hw, C).contiguous().to(self.dev)     # pos_embed + level_embed, [4 hw, C]
        return feat, feat16, pos_lvl

    # ---------------- camera head (decoder.py:39-111, :332-356) -- skipped with skip_camera (decoder.py:437-447)
    def _camera_head(self, enc, feat, pos_lvl):
        w, z, P = self.weights, self.z, self.prog
        B, C, hw, heads, Hn, Wn = self.B, self.C, self.hw, self.heads, self.Hn, self.Wn
        f32 = torch.float32
        Mt, Nc = B * hw, 4 * hw
        self.K33 = z(B, 9, dtype=f32); self.Kinv = z(B, 9, dtype=f32); self.Kpost = z(B, 9, dtype=f32)
        self.Kinv_gt = z(max(self.nb, 1), 9, dtype=f32)
        self.K_gt = z(max(self.nb, 1), 9, dtype=f32)
        if self.skip:
            return
        ct = z(B * 4, C, dtype=f32)
        for j in range(4):
            cj = enc.cls[3 - j]                                             # deepest block first (decoder.py:375-377)
            Cj = cj.shape[1]
            cn = z(_rup(B, 8), Cj, dtype=f32)
            P.layernorm(x=cj, y=cn, rows=B, D=Cj, ldx=Cj, ldy=Cj, eps=1e-5, rows_per_img=B, in_rows_per_img=B, out_rows_per_img=B, out_f32=1)
            P.linear_f32(x=cn, W=w[f"tok.{j}.w"], bias=w[f"tok.{j}.b"], out=ct.data_ptr() + j * C * 4, M=B, N=C, K=Cj, ldx=Cj, ldw=Cj, ldc=4 * C,
                         act=UD_ACT_GELU, tag="cam.tok")
        Mc = B * 4

        def ln32(src, dst, rows=Mc):
            P.layernorm(x=src, y=dst, rows=rows, D=C, ldx=C, ldy=C, eps=1e-5, rows_per_img=rows, in_rows_per_img=rows, out_rows_per_img=rows, out_f32=1)

        def lin32(xb, name, out, n, k, act=UD_ACT_NONE, accumulate=0, **kw):
            P.linear_f32(x=xb, W=w[name + ".w"], bias=w[name + ".b"], out=out, M=Mc, N=n, K=k, ldx=k, ldw=k, ldc=kw.pop("ldc", n), act=act,
                         accumulate=accumulate, tag="cam." + name, **kw)

        def mlp32(pre, stream, out, accumulate, n_out=C):
            nh = w[pre + "fc1.w"].shape[0]
            cn_ = z(Mc, C, dtype=f32); ch_ = z(Mc, nh, dtype=f32)
            ln32(stream, cn_)
            lin32(cn_, pre + "fc1", ch_, nh, C, act=UD_ACT_GELU)
            lin32(ch_, pre + "fc2", out, n_out, nh, accumulate=accumulate)
        cn = z(Mc, C, dtype=f32); c1 = z(Mc, C // 2, dtype=f32); cls_t = z(Mc, C, dtype=f32)
        ln32(ct, cn)
        lin32(cn, "cam.cls1", c1, C // 2, C, act=UD_ACT_GELU)
        lin32(c1, "cam.cls2", cls_t, C, C // 2)
        # features_stack = cat(features, dim=1) + pos_embed  ->  in_features MLP (not residual)  ->  cat with the class tokens
        fsn = z(B * Nc, C)
        for j in range(4):
            P.layernorm(x=feat[j], y=fsn, rows=Mt, D=C, ldx=C, ldy=C, eps=1e-5, rows_per_img=hw, in_rows_per_img=hw, out_rows_per_img=Nc,
                        out_row_off=j * hw, add=pos_lvl)
        hidc = z(B * Nc, 2 * C)
        ctx = z(B * (Nc + 4), C, dtype=f32)
        self._wgemm(fsn, "cam.inf.fc1", hidc, B * Nc, 2 * C, C, epi=UD_EPI_F16, act=UD_ACT_GELU)
        self._wgemm(hidc, "cam.inf.fc2", ctx, B * Nc, C, 2 * C, epi=UD_EPI_F32, rows_in=Nc, rows_out=Nc + 4, row_off=0)
        P.v1(L.UD_V1_COPY_ROWS, a=cls_t, out=ctx, i=(B, 4, Nc + 4, Nc, C, C, 0), tag="cat_cls")
        # aggregate: one head of width C, 4 queries vs 4 hw + 4 keys (decoder.py:94)
        ctxn = z(B * (Nc + 4), C)
        self._ln(ctx, ctxn, B * (Nc + 4), C)
        kvc = z(B * (Nc + 4), 2 * C)
        self._wgemm(ctxn, "cam.agg.kv", kvc, B * (Nc + 4), 2 * C, C, epi=UD_EPI_F16)
        cq = z(Mc, C, dtype=f32); cao = z(Mc, C, dtype=f32)
        ln32(cls_t, cn)
        lin32(cn, "cam.agg.q", cq, C, C, add=w["cam.pos"], ldadd=C, add_mod=4)
        fq_ws = z(B * (-(-(Nc + 4) // 64)) * 4 * (C + 2), dtype=f32)      # key-chunk partials of the few-query attention
        P.v1(L.UD_V1_ATTN_FEWQ, a=cq, b=kvc, c=fq_ws, out=cao, i=(B, 4, Nc + 4, C), f=(C ** -0.5,), tag="cam.aggregate")
        lin32(cao, "cam.agg.out", cls_t, C, C, accumulate=1)
        mlp32("cam.agg.", cls_t, cls_t, 1)
        ckv = z(Mc, 2 * C, dtype=f32)
        for i in range(2):
            ln32(cls_t, cn)                                                 # norm_attnx / norm_attnctx share the statistics
            lin32(cn, f"cam.l{i}.q", cq, C, C, add=w["cam.pos"], ldadd=C, add_mod=4)
            lin32(cn, f"cam.l{i}.kv", ckv, 2 * C, C)
            P.attention_small_f32(cq, ckv, cao, B, 4, heads, C, (C // heads) ** -0.5)
            lin32(cao, f"cam.l{i}.out", cls_t, C, C, accumulate=1)
            mlp32(f"cam.l{i}.", cls_t, cls_t, 1)
        raw = z(Mc, 1, dtype=f32)
        mlp32("cam.out.", cls_t, raw, 0, n_out=1)
        P.v1(L.UD_V1_CAMERA, a=raw, out=self.K33, out2=self.Kinv, c=self.Kpost, i=(B, Hn, Wn, self.pads[0], self.pads[2]), f=(self.ratio,), tag="camera")
        self.tap("intrinsics_net", lambda: self.K33.view(B, 3, 3).clone())

    # ---------------- rays at network resolution (decoder.py:354-355 / unidepthv1.py:334-341 for GT intrinsics) and their
    # spherical-harmonics embeddings at 1/16, 1/8, 1/4 (decoder.py:205-225)
    def _rays_and_embeddings(self):
        z, P, B, C, h, wd, hw, nb, Hn, Wn = self.z, self.prog, self.B, self.C, self.h, self.wd, self.hw, self.nb, self.Hn, self.Wn
        f32 = torch.float32
        self.rays = z(nb, 3, Hn, Wn, dtype=f32)
        P.rays(self.Kinv_gt if self.n_gt else self.Kinv, self.rays, nb, Hn, Wn, 0)
        emb = []
        for hh, ww, Cl, nm in ((h, wd, C, "project_rays16"), (2 * h, 2 * wd, C // 2, "project_rays8"), (4 * h, 4 * wd, C // 4, "project_rays4")):
            n = hh * ww
            sh = z(nb * n, 128)
            P.v1(L.UD_V1_SH_EMBED, a=self.rays, out=sh, i=(nb, Hn, Wn, hh, ww, 128, n), f=(1e-5,), tag="sh_embed")
            hid = z(nb * n, 384)
            e = z(nb * n, Cl, dtype=f32)
            self._wgemm(sh, nm + ".fc1", hid, nb * n, 324, 128, epi=UD_EPI_F16, act=UD_ACT_GELU, ldc=384)
            self._wgemm(hid, nm + ".fc2", e, nb * n, Cl, 384, epi=UD_EPI_F32)
            if nb != B:                                                         # one GT camera for the whole batch: broadcast once, the rest of the program is per image
                eb = z(B * n, Cl, dtype=f32)
                for b in range(B):
                    P.v1(L.UD_V1_COPY_ROWS, a=e, out=eb, i=(1, n, n, b * n, Cl, Cl, 0), tag="bcast")
                e = eb
            emb.append(e)
        self.tap("rays_embedding_16", lambda: emb[0].view(B, hw, C).clone())
        return emb

    # ---------------- latents: channel-concat projection + to_latents MLP (decoder.py:228-235)
    def _latents(self, feat16):
        B, C, hw = self.B, self.C, self.hw
        Mt = B * hw
        lat = self.z(Mt, C, dtype=torch.float32)
        for j in range(4):
            self._wgemm(feat16[j], f"fcat.{j}", lat, Mt, C, C, bias=(j == 0), epi=UD_EPI_F32, accumulate=int(j > 0))
        lat2 = self.z(Mt, C, dtype=torch.float32)
        self._mlp(lat, "tolat.", Mt, C, accumulate=0, out=lat2)
        self.tap("to_latents", lambda: lat2.view(B, hw, C).clone())
        return lat2

    # ---------------- single-head attention of width C via GEMMs: S = Q K^T (fp32), row softmax, O = P V (layers/attention.py:109-142)
    def _big_attn(self, pre, x, ctxn, Nk, add_k=None):
        """x += ls1 * out(softmax(q k^T) v);  x += ls2 * mlp(x).   ctxn: LayerNorm statistics of the context, fp16 [B*Nk, C]."""
        w, z, P, B, C, hw = self.weights, self.z, self.prog, self.B, self.C, self.hw
        Mt = B * hw
        Nkp = _rup(Nk, 64)
        xn = z(Mt, C); q = z(Mt, C); k = z(B * Nk, C); vt = z(B, C, Nkp)
        self._ln(x, xn, Mt, C)
        self._wgemm(xn, pre + "q", q, Mt, C, C, epi=UD_EPI_F16)
        kw = dict(add=add_k, ldadd=C, rows_in=Nk, rows_out=Nk) if add_k is not None else {}
        self._wgemm(ctxn, pre + "k", k, B * Nk, C, C, epi=UD_EPI_F16, **kw)
        # V^T[b] = Wv ctxn[b]^T (operands swapped: no transpose pass); its bias is added after P V (softmax rows sum to one)
        P.gemm(A=w[pre + "v.w"], W=ctxn, out=vt, M=C, N=Nk, ldw=C, ldc=Nkp, epi=UD_EPI_F16, groups=B, gA=0, gW=Nk * C, gOut=C * Nkp,
               tag="v1." + pre + "vT", **_ak(w[pre + "v.w"], C))
        S = z(B * hw, Nk, dtype=torch.float32)
        P.gemm(A=q, W=k, out=S, M=hw, N=Nk, K=C, lda=C, ldw=C, ldc=Nk, epi=UD_EPI_F32, groups=B, gA=hw * C, gW=Nk * C, gOut=hw * Nk, tag="v1." + pre + "qk")
        Pm = z(B * hw, Nkp)
        P.v1(L.UD_V1_SOFTMAX, a=S, out=Pm, i=(B * hw, Nk, Nk, Nkp, 0, 0), f=(1.0,), tag="softmax")
        o = z(Mt, C)
        P.gemm(A=Pm, W=vt, bias=w[pre + "v.b"], out=o, M=hw, N=C, K=Nkp, lda=Nkp, ldw=Nkp, ldc=C, epi=UD_EPI_F16, groups=B, gA=hw * Nkp, gW=C * Nkp,
               gBias=0, gOut=hw * C, tag="v1." + pre + "pv")
        self._wgemm(o, pre + "out", x, Mt, C, C, epi=UD_EPI_F32, accumulate=1)
        self._mlp(x, pre, Mt, C)

    # ---------------- aggregate_16, prompt_camera, layers_16: self-attention, 8 heads of 64, ray embedding added to q (decoder.py:246-247)
    def _layers_16(self, lat, feat, pos_lvl, e16, depth):
        w, z, P, B, C, hw, heads = self.weights, self.z, self.prog, self.B, self.C, self.hw, self.heads
        Mt, Nc = B * hw, 4 * hw
        tokn = z(B * Nc, C)                                                     # LayerNorm statistics of cat(features, dim=1)
        for j in range(4):
            P.layernorm(x=feat[j], y=tokn, rows=Mt, D=C, ldx=C, ldy=C, eps=1e-5, rows_per_img=hw, in_rows_per_img=hw, out_rows_per_img=Nc, out_row_off=j * hw)
        self._big_attn("agg16.", lat, tokn, Nc, add_k=pos_lvl)
        self.tap("aggregate_16", lambda: lat.view(B, hw, C).clone())
        e16n = z(Mt, C)
        self._ln(e16, e16n, Mt, C)
        self._big_attn("pcam.", lat, e16n, hw)
        self.tap("prompt_camera", lambda: lat.view(B, hw, C).clone())
        hwk = _rup(hw, 64)
        for i in range(depth):
            pre = f"l16.{i}."
            xn = z(Mt, C); q = z(Mt, C); k = z(Mt, C); vt = z(B, heads, 64, hwk); ao = z(Mt, C)
            self._ln(lat, xn, Mt, C)
            self._wgemm(xn, pre + "q", q, Mt, C, C, epi=UD_EPI_F16, add=e16, ldadd=C)
            P.gemm(A=xn, W=w[pre + "kv.w"], bias=w[pre + "kv.b"], out=k, out2=vt, M=Mt, N=2 * C, lda=C, ldc=C, epi=UD_EPI_QKV, vsplit=C, **_wk(w[pre + "kv.w"], C),
                   tok_per_img=hw, kv_ld=hwk, heads_v=heads, tag="v1." + pre + "kv")
            P.attention(Q=q, K=k, Vt=vt, O=ao, B=B, H=heads, Nq=hw, Nk=hw, ldq=C, ldk=C, ldo=C, kv_ld=hwk, q_rows_per_img=hw, k_rows_per_img=hw,
                        scale=(C // heads) ** -0.5, tag="v1.l16.attn")
            self._wgemm(ao, pre + "out", lat, Mt, C, C, epi=UD_EPI_F32, accumulate=1)
            self._mlp(lat, pre, Mt, C)
        self.tap("latents_16", lambda: lat.view(B, hw, C).clone())
        self.depth_features_src = (lat, self.h, self.wd, C)

    # ---------------- ConvUpsample (layers/upsample.py:13-45)
    def _conv_upsample(self, nm, x_tok, e_tok, hh, ww, Cl):
        w, z, P, B, zeros = self.weights, self.z, self.prog, self.B, self.zeros
        f32 = torch.float32
        n = hh * ww
        xs = z(B * n, Cl, dtype=f32)
        P.v1(L.UD_V1_ADD, a=x_tok, b=e_tok, out=xs, i=((B * n * Cl) & 0x7fffffff, (B * n * Cl) >> 31), tag="add")
        y = z(B * n, Cl, dtype=f32); xh = z(B * n, Cl); hid = z(B * n, 4 * Cl)
        for c in range(2):
            pre = f"{nm}.{c}."
            P.dwconv7(x=xs, w=w[pre + "dw.w"], bias=w[pre + "dw.b"], y=y, B=B, H=hh, W=ww, C=Cl, ldx=Cl, ldy=Cl, tag="v1.dwconv")
            self._ln(y, xh, B * n, Cl)
            self._wgemm(xh, pre + "fc1", hid, B * n, 4 * Cl, Cl, epi=UD_EPI_F16, act=UD_ACT_GELU)
            self._wgemm(hid, pre + "fc2", xs, B * n, Cl, 4 * Cl, epi=UD_EPI_F32, accumulate=1)
        conv3 = dict(W=w[f"{nm}.up2.w"], bias=w[f"{nm}.up2.b"], zeros=zeros, M=B * 4 * n, N=Cl // 2, ldc=Cl // 2, **_wk(w[f"{nm}.up2.w"], 0, Cl // 2),
                     amode=UD_A_CONV3_ZERO, epi=UD_EPI_F32, Himg=2 * hh, Wimg=2 * ww, coff=0, rows_img=4 * n, tag=f"v1.{nm}.conv3")
        nxt = z(B * 4 * n, Cl // 2, dtype=f32)
        if ASPLIT:
            # three-term tail: [A_hi | A_lo] (fp32 stream split on the way out) x [W_hi | W_hi | W_lo]; the 1x1 conv's output and its
            # align_corners interpolation stay fp32, the 3x3 conv reads the interpolated map as two fp16 terms again
            x16 = z(B * n, 2 * Cl)
            P.v1(L.UD_V1_COPY_ROWS, a=xs, out=x16, i=(1, B * n, B * n, 0, Cl, 2 * Cl, 2), tag="to_f16x2")
            u0 = z(B * n, Cl // 2, dtype=f32)
            P.gemm(A=x16, W=w[f"{nm}.up0.w"], bias=w[f"{nm}.up0.b"], out=u0, M=B * n, N=Cl // 2, lda=2 * Cl, ldc=Cl // 2, epi=UD_EPI_F32, **_wk(w[f"{nm}.up0.w"], Cl),
                   tag=f"v1.{nm}.up0", flops=2.0 * B * n * (Cl // 2) * Cl)
            u1 = z(B * 4 * n, Cl)                                                                                        # [hi | lo] of Cl / 2 channels
            P.v1(L.UD_V1_RESIZE_AC_SPLIT, a=u0, out=u1, i=(B, hh, ww, 2 * hh, 2 * ww, Cl // 2), tag="resize_ac_split")      # UpsamplingBilinear2d = align_corners
            P.gemm(A=u1, out=nxt, cstride=Cl, img_stride=4 * n * Cl, flops=2.0 * B * 4 * n * (Cl // 2) * 9 * (Cl // 2), **conv3)
            return nxt
        x16 = z(B * n, Cl)
        P.v1(L.UD_V1_COPY_ROWS, a=xs, out=x16, i=(1, B * n, B * n, 0, Cl, Cl, 1), tag="to_f16")
        u0 = z(B * n, Cl // 2)
        self._wgemm(x16, f"{nm}.up0", u0, B * n, Cl // 2, Cl, epi=UD_EPI_F16)
        u1 = z(B * 4 * n, Cl // 2)
        P.resize_ac(in_=u0, out=u1, G=1, B=B, Hin=hh, Win=ww, Hout=2 * hh, Wout=2 * ww, C=Cl // 2)                  # UpsamplingBilinear2d = align_corners
        P.gemm(A=u1, out=nxt, cstride=Cl // 2, img_stride=4 * n * (Cl // 2), **conv3)
        return nxt

    def _out_conv(self, nm, x32, hh, ww, Cl):
        # nn.Conv2d(Cl, 1, 3, padding=1) + exp(clamp) (decoder.py:185-187,250-298): one output channel = a stencil over the fp32 map, exact fp32
        # products (rounds 3-4: an MFMA tile padded to 32 columns behind an fp16 [hi | lo] copy of the map: 0.61 + 0.27 ms per infer())
        o = self.z(self.B * hh * ww, 4, dtype=torch.float32)
        self.prog.v1(L.UD_V1_OUT_CONV3, a=x32, b=self.weights[nm + ".cw"], out=o, i=(self.B, hh, ww, Cl, 4), f=(self.weights[f"host.{nm}.bias"],), tag=nm)
        return o

    # ---------------- NystromBlock (layers/nystrom_attention.py:22-84) AS THE REFERENCE EXECUTES IT: q, k, v reach xformers' NystromAttention as
    # [b, n, h, d]; the module reads `seq_len = k.size(-2)` = h (4 / 2), finds num_landmarks (128) >= seq_len and takes its plain-softmax branch
    # over the last two axes -- every token's h head-vectors attend to each other, nothing crosses tokens (oracle/stubs/xformers restates the
    # module statement by statement; rounds 2-4 had built the PAPER's landmark / pseudo-inverse algorithm here, which this layout never reaches).
    def _nystrom_block(self, pre, x, e_tok, n, Cl, nh):
        z = self.z
        M = self.B * n
        xn = z(M, Cl); q = z(M, Cl, dtype=torch.float32); kv = z(M, 2 * Cl, dtype=torch.float32); ao = z(M, Cl)
        self._ln(x, xn, M, Cl)
        self._wgemm(xn, pre + "q", q, M, Cl, Cl, epi=UD_EPI_F32, add=e_tok, ldadd=Cl)
        self._wgemm(xn, pre + "kv", kv, M, 2 * Cl, Cl, epi=UD_EPI_F32)
        self.prog.v1(L.UD_V1_HEAD_MIX, a=q, b=kv, out=ao, i=(M, nh, Cl, 2 * Cl, Cl), f=(64 ** -0.5,), tag="head_mix")
        self._wgemm(ao, pre + "out", x, M, Cl, Cl, epi=UD_EPI_F32, accumulate=1)
        self._mlp(x, pre, M, Cl)

    # ---------------- the three ConvUpsample + 3x3 -> 1 output conv (decoder.py:267-271) + NystromBlock groups
    def _pyramid(self, lat, emb, dec_depths):
        B, C, h, wd, hw, heads = self.B, self.C, self.h, self.wd, self.hw, self.heads
        outs = []
        for lvl, (up, out, layers) in enumerate((("up8", "out8", "layers_8"), ("up4", "out4", "layers_4"), ("up2", "out2", None))):
            m, Cl = 1 << lvl, C >> lvl                      # grid scale and channels going in: (h, wd, C), (2h, 2wd, C/2), (4h, 4wd, C/4)
            lat = self._conv_upsample(up, lat, emb[lvl], m * h, m * wd, Cl)
            self.tap(up, lambda t=lat, m=m, Cl=Cl: t.view(B, 4 * m * m * hw, Cl // 2).clone())
            outs.append(self._out_conv(out, lat, 2 * m * h, 2 * m * wd, Cl // 2))
            if layers:
                for i in range(dec_depths[lvl + 1]):
                    self._nystrom_block(f"{layers}.{i}.", lat, emb[lvl + 1], 4 * m * m * hw, Cl // 2, heads >> (lvl + 1))
                self.tap(layers, lambda t=lat, m=m, Cl=Cl: t.view(B, 4 * m * m * hw, Cl // 2).clone())
        for o, nm, m in zip(outs, ("out8", "out4", "out2"), (2, 4, 8)):
            self.tap(nm, lambda o=o, m=m: o.view(B, m * h, m * wd, 4)[..., 0].clone())
        return outs

    # ---------------- multi-scale mean at network resolution, pad crop + resize to the input size (unidepthv1.py:66-86)
    def _merge_and_postprocess(self, outs):
        z, P, B, H, W, Hn, Wn, h, wd = self.z, self.prog, self.B, self.H, self.W, self.Hn, self.Wn, self.h, self.wd
        pl, pr, pt, pb = self.pads
        f32 = torch.float32
        rs = []
        for o, m in zip(outs, (2, 4, 8)):
            r = z(B * Hn * Wn, 4, dtype=f32)
            P.v1(L.UD_V1_RESIZE_AA, a=o, out=r, i=(B, m * h, m * wd, Hn, Wn, 4, 4, 4, 0, 0, m * h, m * wd), tag="resize_aa")
            rs.append(r)
        pred = z(B * Hn * Wn, 4, dtype=f32)
        P.v1(L.UD_V1_MEAN3, a=rs[0], b=rs[1], c=rs[2], out=pred, i=((B * Hn * Wn) & 0x7fffffff, 4, (B * Hn * Wn) >> 31), tag="mean3")
        self.zout = z(B * H * W, 4, dtype=f32)
        P.v1(L.UD_V1_RESIZE_AA, a=pred, out=self.zout, i=(B, Hn, Wn, H, W, 4, 4, 4, pt, pl, Hn - pt - pb, Wn - pl - pr), tag="resize_aa")
