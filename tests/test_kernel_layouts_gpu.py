"""Kernels at strided, offset layouts with guarded outputs (tests/layout_guard.py).

Every case runs through the `ops` entry points with inputs at a row stride wider than their width (padding poisoned with NaN, rows past
the logical extent poisoned), outputs at a non-zero row / column offset inside a sentinel-filled allocation with ld > width, and is
judged element by element against the fp64 statement of the op on the same fp16-rounded operands, plus a BITWISE check of every guard
element.  A GEMM case also runs at the product's own (dense) layout: both runs must agree bit for bit, so only the layout changed.

GEMM_CASES is the matrix of GEMM schedules this module covers; each case names the ud_gemm_pick value it reaches (asserted here and, on
the host, by tests/test_layout_coverage_cpu.py, which also checks that every GEMM descriptor of the recorded V1 / V2 plans -- single-image
and batched -- falls into a class of this table).  Every run prints `RATIO gemm <case> <layout> <worst error / bound>`.  The module imports without a GPU."""
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(os.path.dirname(os.path.abspath(__file__)), "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)

pytestmark = pytest.mark.gpu

F16, F32, QKV, D2S, HEAD = 0, 1, 2, 3, 4
GELU, LRELU = 1, 2

# ---- the GEMM matrix ------------------------------------------------------------------------------------------------------------------
# keys: M N K epi act act2 acc(umulate) out2 hint groups gap (rows between group outputs) gA0 (A shared by the groups) a_wrap w_wrap
#       remap (rows_in, rows_out, row_off) add lnin (row_stats_in) rso (row_stats_out) rsf (row_stats_final) maxo splitk (1 small / 2 large)
#       conv: amode Cin H W B pad (rows past H*W per image); qkv: B heads; d2s: k B Hin Win pad; head: B H W Hs Ws (amode 3)
#       lay: layouts run, (A strided, C strided) pairs; the first is the reference of the bit-identity check
_L2 = ((0, 0), (1, 1))
GEMM_CASES = [
    # 128-row kernels, BN 128 / 64 / 32 (picks 0 / 1 / 2): partial M and N tiles, N % 64 != 0
    dict(id="bn128_f16", pick=0, M=300, N=196, K=64, act=GELU),
    dict(id="bn128_f16_wrap", pick=0, M=1064, N=324, K=256, act=GELU, a_wrap=128),
    dict(id="bn128_f32_acc1_out2", pick=0, M=1000, N=388, K=320, epi=F32, acc=1, out2=1, act2=LRELU),
    dict(id="bn128_f32_acc0_gelu", pick=0, M=333, N=260, K=128, epi=F32, act=GELU),
    dict(id="bn128_f32_acc2_out2", pick=0, M=333, N=260, K=128, epi=F32, acc=2, out2=1),
    dict(id="bn128_f32_wrap", pick=0, M=1777, N=192, K=128, epi=F32, a_wrap=64),
    dict(id="bn128_f32_maxo", pick=0, M=301, N=256, K=128, epi=F32, maxo=1),
    dict(id="bn128_f16_groups_gap", pick=0, M=700, N=196, K=256, groups=3, gap=8),
    dict(id="bn128_f32_groups_gap", pick=0, M=700, N=256, K=192, epi=F32, groups=4, gap=8),
    dict(id="bn64_f32", pick=1, M=1555, N=64, K=128, epi=F32),
    dict(id="bn64_f32_wrap", pick=1, M=1555, N=60, K=384, epi=F32, a_wrap=256),
    dict(id="bn32_f16", pick=2, M=277, N=28, K=192),
    dict(id="bn128_qkv", pick=0, M=2 * 300, N=3 * 128, K=192, epi=QKV, B=2, heads=2),
    dict(id="bn128_qkv_groups", pick=0, M=2 * 200, N=3 * 128, K=128, epi=QKV, B=2, heads=2, groups=2, gA0=1),
    dict(id="hint1_f16", pick=0, M=1100, N=516, K=128, hint=1, act=GELU),
    dict(id="hint5_plain_f32", pick=0, M=700, N=516, K=1024, hint=5, epi=F32, acc=1),
    # 128x128 4-stage ring (6) and its two-way K split (7)
    dict(id="ring_f16", pick=6, M=1064, N=516, K=512),
    dict(id="ring_f16_wrap", pick=6, M=1064, N=772, K=1536, act=GELU, a_wrap=768),
    dict(id="ring_f16_remap_add_wrap", pick=6, M=1000, N=256, K=1024, a_wrap=512, remap=(500, 509, 3), add=1),
    dict(id="ring_f16_wwrap", pick=6, M=512, N=1064, K=1024, w_wrap=512, lay=((0, 0), (0, 1), (1, 1))),
    dict(id="ring_f32", pick=6, M=1064, N=516, K=512, epi=F32),
    dict(id="ring_f32_remap_add", pick=6, M=1452, N=384, K=640, epi=F32, acc=1, remap=(726, 728, 1), add=1),
    dict(id="ring_f32_wrap_out2", pick=6, M=1064, N=516, K=768, epi=F32, act=GELU, out2=1, a_wrap=384),
    dict(id="ring_f32_remap_wrap", pick=6, M=1000, N=512, K=2048, epi=F32, a_wrap=1024, remap=(1000, 1004, 0)),
    dict(id="ring_qkv_wrap", pick=6, M=1064, N=3 * 256, K=1024, epi=QKV, B=1, heads=4, a_wrap=512),
    dict(id="ksplit_f32", pick=7, M=1456, N=384, K=1536, epi=F32, acc=1, splitk=1),
    dict(id="ksplit_f32_wrap", pick=7, M=1000, N=388, K=1536, epi=F32, a_wrap=768, splitk=1),
    dict(id="ksplit_f16_wrap", pick=7, M=1064, N=1020, K=1024, act=GELU, a_wrap=512, splitk=1),
    dict(id="ksplit_f16_wwrap", pick=7, M=512, N=1064, K=1024, w_wrap=512, splitk=1, lay=((0, 0), (0, 1), (1, 1))),
    dict(id="hint7_f16", pick=7, M=700, N=516, K=512, hint=7, splitk=1),
    # the two classes only the V1 ViT-L plan records: the split-fp16 token projection behind the row remap (K split), the split-fp16 qkv on plain tiles
    dict(id="ksplit_f32_remap_add_wrap", pick=7, M=1000, N=384, K=1280, epi=F32, a_wrap=640, remap=(500, 509, 3), add=1, splitk=1),
    dict(id="bn128_qkv_wrap", pick=0, M=1064, N=3 * 256, K=1024, epi=QKV, B=1, heads=4, a_wrap=512, hint=5),
    # large tiles: 256x256 (2 -> 4), 192x256 (3), row-balanced (8), 2-deep weight ring (9 -> 3), large-tile K split (10)
    dict(id="hint2_f16_gelu", pick=4, M=1100, N=516, K=128, hint=2, act=GELU),
    dict(id="hint2_f32_acc1_out2", pick=4, M=1100, N=516, K=384, hint=2, epi=F32, acc=1, out2=1),
    dict(id="hint3_f16", pick=3, M=1300, N=772, K=384, hint=3),
    dict(id="hint3_f32_remap", pick=3, M=1200, N=512, K=256, hint=3, epi=F32, acc=1, remap=(600, 603, 1), add=1),
    dict(id="hint3_qkv", pick=3, M=2 * 700, N=3 * 256, K=256, hint=3, epi=QKV, B=2, heads=4),
    dict(id="hint8_f16", pick=8, M=11000, N=1024, K=256, hint=8),
    dict(id="hint8_f32_acc1", pick=8, M=11000, N=1024, K=256, hint=8, epi=F32, acc=1, out2=1),
    dict(id="hint9_f16", pick=3, M=1300, N=772, K=384, hint=9),
    dict(id="hint10_f16", pick=10, M=3000, N=1024, K=2048, hint=10, splitk=2),
    dict(id="conv_zero_ksplit_f16", pick=10, amode=1, M=0, N=256, K=2304, Cin=256, H=132, W=176, B=1, pad=0, act=LRELU, splitk=2),
    dict(id="conv_zero_ksplit_f32_out2", pick=10, amode=1, M=0, N=256, K=2304, Cin=256, H=132, W=176, B=1, pad=0, epi=F32, acc=1, out2=1, act2=LRELU,
         splitk=2),
    # ping-pong (11), two workgroups per CU (12-14)
    dict(id="pingpong_f32", pick=11, M=11008 - 40, N=1024, K=512, epi=F32, acc=1, out2=1, act2=LRELU),
    dict(id="hint11_f32", pick=11, M=1100, N=512, K=256, hint=11, epi=F32),
    dict(id="duo12_f32", pick=12, M=1100, N=512, K=256, hint=12, epi=F32, acc=1),
    dict(id="duo13_f32", pick=12, M=1100, N=512, K=256, hint=13, epi=F32, out2=1),
    dict(id="duo14_f32", pick=12, M=1100, N=512, K=384, hint=14, epi=F32, acc=1),
    # grouped problem as one large-tile list (36), LayerNorm-folded consumer (+16), row statistics producer
    dict(id="grouped_as_one_f16", pick=36, M=2816, N=1024, K=512, groups=4, act=GELU),
    dict(id="grouped_as_one_qkv", pick=36, M=2816, N=3 * 256, K=512, epi=QKV, B=1, heads=4, groups=4, gA0=1),
    dict(id="lnfold_consumer_wrap", pick=20, M=17710, N=768, K=384, act=GELU, a_wrap=192, lnin=1),
    dict(id="lnfold_consumer_hint3", pick=19, M=1300, N=1024, K=256, hint=3, act=GELU, lnin=1),
    dict(id="lnfold_consumer_qkv", pick=19, M=1300, N=3 * 256, K=256, hint=3, epi=QKV, B=1, heads=4, lnin=1),
    dict(id="rowstats_producer_final", pick=3, M=1300, N=512, K=256, hint=3, epi=F32, acc=1, out2=1, rso=1, rsf=1),
    dict(id="rowstats_producer_hint2", pick=4, M=1100, N=256, K=128, hint=2, epi=F32, acc=1, out2=1, rso=1),
    # implicit-GEMM convolutions: 128-row kernels (0 / 1), halo-tile kernel (5), the D2S and HEAD epilogues
    dict(id="conv_zero_f16", pick=0, amode=1, M=0, N=128, K=576, Cin=64, H=9, W=11, B=2, pad=5, act=LRELU),
    dict(id="conv_zero_f32_acc1_out2", pick=0, amode=1, M=0, N=256, K=1152, Cin=128, H=13, W=17, B=2, pad=3, epi=F32, acc=1, out2=1, act2=LRELU),
    dict(id="conv_zero_f32_wrap", pick=0, amode=1, M=0, N=256, K=1728, Cin=192, H=12, W=11, B=1, pad=4, epi=F32, a_wrap=128),
    dict(id="conv_zero_f32_bn64_wrap", pick=1, amode=1, M=0, N=64, K=1728, Cin=192, H=40, W=31, B=1, pad=0, epi=F32, a_wrap=128),
    dict(id="conv_reflect_f16", pick=0, amode=2, M=0, N=128, K=576, Cin=64, H=10, W=7, B=2, pad=3),
    dict(id="conv_halo_f16_groups", pick=5, amode=2, M=0, N=32, K=576, Cin=64, H=40, W=33, B=1, pad=0, groups=2, act=LRELU),
    dict(id="conv_halo_f16_n64", pick=5, amode=1, M=0, N=64, K=1152, Cin=128, H=37, W=21, B=1, pad=0),
    dict(id="d2s_k1", pick=0, epi=D2S, M=0, N=256, K=256, k=1, B=2, Hin=9, Win=11, pad=3, out2=1, act2=LRELU),
    dict(id="d2s_k2", pick=0, epi=D2S, M=0, N=4 * 128, K=128, k=2, B=2, Hin=7, Win=9, pad=4, out2=1, act2=LRELU),
    dict(id="head_reflect_groups", pick=2, epi=HEAD, amode=2, M=0, N=32, K=320, Cin=32, H=20, W=13, B=1, pad=0, groups=2),
    dict(id="head_reflect_up_groups", pick=5, epi=HEAD, amode=3, M=0, N=32, K=576, Cin=64, H=46, W=61, Hs=26, Ws=35, B=1, pad=0, groups=2),
    # ---- the classes only the BATCHED plans record (tests/test_layout_coverage_cpu.py SIGNATURES: M = B x tokens moves the tile choice).
    # A wrap boundary is an odd multiple of 64 wherever a wrap meets a row remap or groups: it then falls inside the 128-wide K step of the
    # large-tile kernels, in a launch whose remapped image boundary falls inside a row tile.
    # 128-row kernels: V1 at batch 2 (split-fp16 token projections behind the row remap), the ViT-B head convolutions (Cin 96, N 48, two branches),
    # the grouped prompt projection with the split-fp16 weight operand, V2 ViT-S at batch 8 (the token projection behind the row remap)
    dict(id="bn128_f16_remap_add_wrap", pick=0, M=1000, N=324, K=384, a_wrap=192, remap=(500, 509, 3), add=1),
    dict(id="bn128_f32_remap_wrap", pick=0, M=1000, N=260, K=384, epi=F32, a_wrap=192, remap=(500, 504, 0)),
    dict(id="bn128_f32_remap_add", pick=0, M=1000, N=260, K=320, epi=F32, remap=(500, 504, 1), add=1),
    dict(id="bn128_f16_groups_wwrap", pick=0, M=300, N=324, K=640, w_wrap=320, groups=2, gA0=1, lay=((0, 0), (0, 1), (1, 1))),
    dict(id="conv_reflect_bn64_groups", pick=1, amode=2, M=0, N=48, K=896, Cin=96, H=13, W=11, B=2, pad=0, groups=2),
    dict(id="ring_qkv", pick=6, M=1064, N=3 * 256, K=512, epi=QKV, B=1, heads=4),
    # 192 x 256 tile list: split-fp16 A on every epilogue, implicit-GEMM convolutions, D2S
    dict(id="hint3_f16_wrap", pick=3, M=1300, N=772, K=384, hint=3, act=GELU, a_wrap=192),
    dict(id="hint3_f16_remap_add_wrap", pick=3, M=1200, N=516, K=640, hint=3, a_wrap=320, remap=(600, 603, 1), add=1),
    dict(id="hint3_f32_wrap_acc1_maxo", pick=3, M=1300, N=516, K=384, hint=3, epi=F32, acc=1, maxo=1, a_wrap=192),
    dict(id="hint3_f32_wrap_gelu_out2", pick=3, M=1300, N=516, K=384, hint=3, epi=F32, act=GELU, out2=1, a_wrap=192),
    dict(id="hint3_f32_remap_add_wrap", pick=3, M=1200, N=516, K=640, hint=3, epi=F32, a_wrap=320, remap=(600, 603, 1), add=1),
    dict(id="hint3_qkv_wrap", pick=3, M=2 * 700, N=3 * 256, K=512, hint=3, epi=QKV, B=2, heads=4, a_wrap=256),
    dict(id="hint3_conv_zero_f16", pick=3, amode=1, M=0, N=320, K=576, Cin=64, H=20, W=27, B=2, pad=4, hint=3, act=LRELU),
    dict(id="hint3_conv_zero_f32_acc1_out2", pick=3, amode=1, M=0, N=320, K=576, Cin=64, H=20, W=27, B=2, pad=4, hint=3, epi=F32, acc=1, out2=1, act2=LRELU),
    dict(id="hint3_conv_zero_f32_acc2_out2", pick=3, amode=1, M=0, N=320, K=576, Cin=64, H=20, W=27, B=2, pad=4, hint=3, epi=F32, acc=2, out2=1),
    dict(id="hint3_conv_zero_f32_wrap", pick=3, amode=1, M=0, N=320, K=1728, Cin=192, H=20, W=27, B=2, pad=4, hint=3, epi=F32, a_wrap=128),
    # D2S: Co % 64 == 0 takes the straight-line epilogue on full tiles (k >= 2 then has no partial column tile: k k Co % 256 == 0), any other Co the
    # element-wise one on every tile
    dict(id="hint3_d2s_k1", pick=3, epi=D2S, M=0, N=320, K=256, k=1, B=2, Hin=20, Win=27, pad=4, hint=3, out2=1, act2=LRELU),
    dict(id="hint3_d2s_k2", pick=3, epi=D2S, M=0, N=4 * 192, K=128, k=2, B=2, Hin=20, Win=27, pad=4, hint=3, out2=1, act2=LRELU),
    dict(id="hint3_d2s_k2_co80", pick=3, epi=D2S, M=0, N=4 * 80, K=128, k=2, B=2, Hin=20, Win=27, pad=4, hint=3, out2=1, act2=LRELU),
    # 256 x 256 tile list
    dict(id="hint2_f16_wrap", pick=4, M=1100, N=516, K=384, hint=2, act=GELU, a_wrap=192),
    dict(id="hint2_f16_remap_add_wrap", pick=4, M=1200, N=516, K=640, hint=2, a_wrap=320, remap=(600, 603, 1), add=1),
    dict(id="hint2_f32_remap_add", pick=4, M=1200, N=516, K=640, hint=2, epi=F32, remap=(600, 612, 1), add=1),
    dict(id="hint2_f32_wrap_acc1_maxo", pick=4, M=1100, N=516, K=384, hint=2, epi=F32, acc=1, maxo=1, a_wrap=192),
    dict(id="hint2_f32_remap_wrap", pick=4, M=1200, N=516, K=640, hint=2, epi=F32, a_wrap=320, remap=(600, 604, 0)),
    dict(id="hint2_qkv", pick=4, M=2 * 700, N=3 * 256, K=256, hint=2, epi=QKV, B=2, heads=4),
    dict(id="hint2_conv_zero_f16", pick=4, amode=1, M=0, N=320, K=576, Cin=64, H=20, W=27, B=2, pad=4, hint=2, act=LRELU),
    dict(id="hint2_conv_zero_f32_acc1_out2", pick=4, amode=1, M=0, N=320, K=576, Cin=64, H=20, W=27, B=2, pad=4, hint=2, epi=F32, acc=1, out2=1, act2=LRELU),
    dict(id="hint2_conv_zero_f32_acc2_out2", pick=4, amode=1, M=0, N=320, K=576, Cin=64, H=20, W=27, B=2, pad=4, hint=2, epi=F32, acc=2, out2=1),
    dict(id="hint2_d2s_k2", pick=4, epi=D2S, M=0, N=4 * 192, K=128, k=2, B=2, Hin=20, Win=27, pad=4, hint=2, out2=1, act2=LRELU),
    dict(id="hint2_d2s_k4_co20", pick=4, epi=D2S, M=0, N=16 * 20, K=128, k=4, B=2, Hin=20, Win=27, pad=4, hint=2, out2=1, act2=LRELU),
    dict(id="lnfold_consumer_hint2", pick=20, M=1100, N=528, K=256, hint=2, act=GELU, lnin=1),
    # row-balanced schedule (N % 256 == 0, at least two 64-row units per workgroup): split-fp16 A, convolutions, QKV, the LayerNorm fold
    dict(id="hint8_f16_wrap", pick=8, M=11000, N=1024, K=384, hint=8, act=GELU, a_wrap=192),
    dict(id="hint8_f32_wrap_acc1", pick=8, M=11000, N=1024, K=384, hint=8, epi=F32, acc=1, a_wrap=192),
    dict(id="hint8_f32_wrap_add", pick=8, M=11000, N=1024, K=384, hint=8, epi=F32, a_wrap=192, add=1),
    dict(id="hint8_qkv", pick=8, M=2 * 5460, N=3 * 256, K=256, hint=8, epi=QKV, B=2, heads=4),
    dict(id="hint8_qkv_wrap", pick=8, M=2 * 5460, N=3 * 256, K=384, hint=8, epi=QKV, B=2, heads=4, a_wrap=192),
    dict(id="hint8_conv_zero_f16", pick=8, amode=1, M=0, N=1024, K=576, Cin=64, H=59, W=70, B=2, pad=4, hint=8, act=LRELU),
    dict(id="hint8_conv_zero_f32_acc1_out2", pick=8, amode=1, M=0, N=1024, K=576, Cin=64, H=59, W=70, B=2, pad=4, hint=8, epi=F32, acc=1, out2=1, act2=LRELU),
    dict(id="hint8_conv_zero_f32_acc2_out2", pick=8, amode=1, M=0, N=1024, K=576, Cin=64, H=59, W=70, B=2, pad=4, hint=8, epi=F32, acc=2, out2=1),
    dict(id="hint8_conv_zero_f32_wrap", pick=8, amode=1, M=0, N=1024, K=1728, Cin=192, H=59, W=70, B=2, pad=4, hint=8, epi=F32, a_wrap=128),
    dict(id="lnfold_consumer_hint8", pick=24, M=11000, N=1024, K=256, hint=8, act=GELU, lnin=1),
    dict(id="lnfold_consumer_hint8_wrap", pick=24, M=11000, N=1024, K=384, hint=8, act=GELU, a_wrap=192, lnin=1),
    dict(id="lnfold_consumer_hint8_qkv", pick=24, M=2 * 5460, N=3 * 256, K=256, hint=8, epi=QKV, B=2, heads=4, lnin=1),
    # large-tile K split and the grouped problem as one tile list, fp32 epilogue (ViT-L at batch 4 / 8 / 32)
    dict(id="hint10_f32_acc1", pick=10, M=3000, N=1024, K=2048, hint=10, epi=F32, acc=1, splitk=2),
    dict(id="grouped_as_one_f32", pick=36, M=2816, N=1024, K=1024, epi=F32, groups=4),
]


def _lay(c):
    return c.get("lay", _L2)


def _vcols(n):
    t = torch.arange(n)
    return (t & ~15) | ((t & 4) << 1) | ((t & 8) >> 1) | (t & 3)


def gemm_scalars(c, lay):
    """Scalar descriptor fields of case `c` at layout `lay` (pa: A / W strided, pc: outputs strided), plus the pointer fields it sets."""
    pa, pc = lay
    epi, amode, G = c.get("epi", F16), c.get("amode", 0), c.get("groups", 1)
    N, K = c["N"], c["K"]
    s = dict(N=N, K=K, epi=epi, amode=amode, act=c.get("act", 0), act2=c.get("act2", 0), accumulate=c.get("acc", 0), tile_hint=c.get("hint", 0))
    ptrs = {"A", "W", "out", "bias"}
    if amode:
        cin_st = c.get("a_wrap") or c["Cin"]
        cst = cin_st + (16 if pa else 0)
        hw = c["H"] * c["W"]
        rows_img = hw + c["pad"]
        s.update(Cin=c["Cin"], Himg=c["H"], Wimg=c["W"], cstride=cst, coff=8 if pa else 0, rows_img=rows_img, lda=0)
        ptrs.add("zeros")
        if amode == 3:
            s.update(Hsrc=c["Hs"], Wsrc=c["Ws"], img_stride=c["Hs"] * c["Ws"] * cst + (64 if pa else 0))
        else:
            s["img_stride"] = rows_img * cst + (64 if pa else 0)
        s["M"] = c["B"] * rows_img
    elif epi == D2S:
        s["M"] = c["B"] * (c["Hin"] * c["Win"] + c["pad"])
        s["lda"] = K + (64 if pa else 0)
    else:
        s["M"] = c["M"]
        s["lda"] = (c.get("a_wrap") or K) + (64 if pa else 0)
    s["ldw"] = (c.get("w_wrap") or K) + (64 if pa else 0)
    if c.get("a_wrap"):
        s["a_wrap"] = c["a_wrap"]
    if c.get("w_wrap"):
        s["w_wrap"] = c["w_wrap"]
    M = s["M"]
    if epi in (F16, F32):
        s["ldc"] = N + (256 if pc else 0)
    elif epi == QKV:
        D = N // 3
        s.update(ldc=2 * D + (256 if pc else 0), vsplit=2 * D, tok_per_img=M // c["B"], heads_v=c["heads"], kv_ld=(M // c["B"] + 63) // 64 * 64 + (64 if pc else 0))
        ptrs.add("out2")
    elif epi == D2S:
        k, Co = c["k"], N // (c["k"] ** 2)
        s.update(ldc=Co + (256 if pc else 0), d2s_k=k, d2s_Co=Co, d2s_Hin=c["Hin"], d2s_Win=c["Win"], d2s_rows_in_img=c["Hin"] * c["Win"] + c["pad"],
                 d2s_out_img_pix=c["Hin"] * c["Win"] * k * k + (5 if pc else 0))
    else:
        s.update(ldc=0, b2=0.1, post_add=1.0, b2_g1=-0.2, post_add_g1=0.0)
        ptrs.add("w2")
    if c.get("out2") and epi in (F32, D2S):
        s["ldc2"] = s["ldc"] + (64 if pc else 0)
        ptrs.add("out2")
    if c.get("remap"):
        s["rows_in"], s["rows_out"], s["row_off"] = c["remap"]
    if c.get("add"):
        s["ldadd"] = N + (64 if pa else 0)
        if c.get("remap"):
            s["add_row_off"] = 1
        ptrs.add("add")
    if G > 1:
        s["groups"] = G
        a_rows = M if amode == 0 else None
        s["gA"] = 0 if c.get("gA0") else (a_rows * s["lda"] if amode == 0 else (s["img_stride"] * c["B"] + (128 if pa else 0)))
        s["gW"] = (N + (8 if pa else 0)) * s["ldw"]
        s["gBias"] = N + (8 if pa else 0)
        if epi == HEAD:
            s["gOut"] = M + (256 if pc else 0)
            s["gW2"] = 32 + (8 if pa else 0)
        else:
            s["gOut"] = (M + c.get("gap", 0) * pc) * s["ldc"]
        if epi == QKV:
            s["gOut2"] = c["B"] * c["heads"] * 64 * s["kv_ld"]
        elif "out2" in ptrs:
            s["gOut2"] = (M + c.get("gap", 0) * pc) * s["ldc2"]
    if c.get("lnin"):
        ptrs |= {"row_stats_in", "wsum"}
        s.update(ln_D=K, ln_eps=1e-6)
    if c.get("rso"):
        ptrs.add("row_stats_out")
        if c.get("rsf"):
            ptrs |= {"row_stats_final", "row_stats_ticket"}
            s.update(ln_D=N, ln_eps=1e-6)
    if c.get("maxo"):
        ptrs.add("max_out")
        s["max_init"] = 0
    if c.get("splitk"):
        ptrs |= {"splitk_ws", "splitk_cnt"}
        if c["splitk"] == 2:
            tiles192 = -(-M // 192) * -(-N // 256)
            s["splitk_ws_bytes"] = 2 * tiles192 * 192 * 256 * 4
    return s, ptrs


def gemm_class(d):
    """The coverage class of a UdGemm descriptor (tests/test_layout_coverage_cpu.py): schedule, epilogue, A mode and the layout flags."""
    from unidepth_amd import _lib
    return (_lib.lib.ud_gemm_pick(C.byref(d)), d.epi, d.amode, d.lda != d.K, d.ldc != d.N, d.rows_in != 0, d.groups > 1,
            bool(d.a_wrap or d.w_wrap), bool(d.row_stats_in))


def host_desc(c, lay):
    """The case's descriptor with placeholder addresses (schedule selection reads only sizes and which pointers are set)."""
    from unidepth_amd import _lib
    s, ptrs = gemm_scalars(c, lay)
    d = _lib.UdGemm()
    for k, v in s.items():
        setattr(d, k, v)
    for k in ptrs:
        setattr(d, k, 0x10000)
    return d


def declared_gemm_classes():
    return {gemm_class(host_desc(c, lay)) for c in GEMM_CASES for lay in _lay(c)}


# linear_f32 / layernorm / attention: the stride flags the cases below cover (tests/test_layout_coverage_cpu.py)
LINEAR_F32_FLAGS = {(ldx_pad, ldc_pad, add) for ldx_pad in (False, True) for ldc_pad in (False, True) for add in (False, True)}
LAYERNORM_FLAGS = {(ldx_pad, ldy_pad, remap, cls, f32, add) for ldx_pad, ldy_pad in ((False, False), (True, True)) for remap in (False, True)
                   for cls, f32, add in ((False, False, False), (True, False, False), (False, True, False), (False, False, True))}
ATTENTION_FLAGS = None        # set below from ATT_CASES
ATTENTION_SCHEDULES = None    # set below from ATT_CASES and the case table of tests/test_attention_paths_gpu.py


def _attention_schedule(B, H, Nq, Nk, pre):
    """What the attention kernels' control flow depends on besides the strides.  The pipelined kernel (pre-scaled Q): ("pipe", the steady
    two-tile loop is taken, rem = the 1 .. 3 tiles after it, the last tile has a key tail, walk = more items per XCD than its 64 persistent
    workgroups, fewer (image, head) pairs than XCDs).  The one-tile kernel (raw Q): ("tile", one tile only, key tail)."""
    nt, tail = (Nk + 63) // 64, Nk % 64 != 0
    if not pre:
        return ("tile", nt == 1, tail)
    t = 0
    while t + 4 <= nt:
        t += 2
    pairs, qt = B * H, (Nq + 127) // 128
    return ("pipe", t > 0, nt - t, tail, (pairs + 7) // 8 * qt > 64, pairs < 8)


def attention_schedule(d):
    return _attention_schedule(d.B, d.H, d.Nq, d.Nk, bool(d.q_prescaled))


def linear_flags(d):
    return (d.ldx != d.K, d.ldc != d.N, bool(d.add))


def layernorm_flags(d):
    return (d.ldx != d.D, d.ldy != d.D, d.out_rows_per_img != d.rows_per_img or d.in_rows_per_img != d.rows_per_img or d.out_row_off != 0,
            bool(d.cls_y), bool(d.out_f32), bool(d.add))


def attention_flags(d):
    return (d.ldq != d.H * 64, d.ldk != d.H * 64, d.ldo != d.H * 64, d.q_rows_per_img != d.Nq or d.k_rows_per_img != d.Nk, bool(d.kv_broadcast),
            bool(d.q_prescaled))


# ---- GPU side ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unidepth_amd import ops as _ops
    return _ops


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _act(x, a):
    return F.gelu(x) if a == GELU else F.leaky_relu(x, 0.01) if a == LRELU else x


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _conv_rows(img, c, s, g):
    """fp64 im2col rows [B*rows_img, K] of the case's 3x3 convolution (k = tap * Cin + cin; rows past H*W are zero)."""
    B, H, W, Cin = c["B"], c["H"], c["W"], c["Cin"]
    x = img[g]                                                                    # [B, H, W, Cin] fp64 (wrapped channels already resolved)
    x = x.permute(0, 3, 1, 2)
    if c["amode"] >= 2:
        x = F.pad(x, (1, 1, 1, 1), mode="reflect")
    else:
        x = F.pad(x, (1, 1, 1, 1))
    u = F.unfold(x, 3).view(B, Cin, 9, H * W).permute(0, 3, 2, 1).reshape(B, H * W, 9 * Cin)
    rows = torch.zeros(B, s["rows_img"], s["K"], dtype=torch.float64, device=x.device)
    rows[:, :H * W, :9 * Cin] = u
    return rows.reshape(-1, s["K"])


def run_gemm(ops, c, lay, seed=0):
    """Run case `c` at layout `lay`; returns {name: output view} after checking every element and every guard."""
    s, ptrs = gemm_scalars(c, lay)
    pa, pc = lay
    epi, amode, G = s["epi"], s["amode"], s.get("groups", 1)
    M, N, K = s["M"], s["N"], s["K"]
    dev = "cuda"
    kw = dict(s)
    # ---- operands
    GA = 1 if (s.get("gA", 1) == 0 and G > 1) else G
    if amode == 0:
        acols = s.get("a_wrap") or K
        A = _rnd((GA, M, acols), seed + 1).half()
        if epi == D2S:                                                            # input rows past Hin*Win of an image: poison (never read)
            A.view(GA, c["B"], -1, acols)[:, :, c["Hin"] * c["Win"]:] = float("nan")
        Ab = lg.poisoned(A.reshape(GA * M, acols), ld=s["lda"], post_rows=64 if pa else 0)
        kw["A"] = Ab
        Aeff = A if not s.get("a_wrap") else torch.cat([A, A[..., :K - acols]], -1)
        Arows = [Aeff[min(g, GA - 1)].double() for g in range(G)]
    else:
        Cst, cst = s.get("a_wrap") or c["Cin"], s["cstride"]
        Hs, Ws = (c["Hs"], c["Ws"]) if amode == 3 else (c["H"], c["W"])
        pix = Hs * Ws if amode == 3 else s["rows_img"]
        img = _rnd((G, c["B"], pix, Cst), seed + 1).half()
        flat = torch.full((G * s.get("gA", 0) + c["B"] * s["img_stride"] + 4096,), float("nan"), dtype=torch.half, device=dev)
        gA = s.get("gA", c["B"] * s["img_stride"])
        for g in range(G):
            for b in range(c["B"]):
                base = g * gA + b * s["img_stride"]
                flat[base:base + pix * cst].view(pix, cst)[:, s["coff"]:s["coff"] + Cst] = img[g, b]
        if amode != 3:
            img_in = img.clone()
            img_in[:, :, c["H"] * c["W"]:] = float("nan")                        # rows past H*W: poison (never read)
            for g in range(G):
                for b in range(c["B"]):
                    base = g * gA + b * s["img_stride"]
                    flat[base:base + pix * cst].view(pix, cst)[:, s["coff"]:s["coff"] + Cst] = img_in[g, b]
        kw["A"] = flat
        zeros = torch.zeros(256, dtype=torch.half, device=dev)
        kw["zeros"] = zeros
        x = img.double()
        if s.get("a_wrap"):
            x = torch.cat([x, x[..., :c["Cin"] - Cst]], -1)
        if amode == 3:
            up = F.interpolate(x.view(G * c["B"], Hs, Ws, c["Cin"]).permute(0, 3, 1, 2), size=(c["H"], c["W"]), mode="bilinear", align_corners=True)
            x = up.permute(0, 2, 3, 1).reshape(G, c["B"], c["H"], c["W"], c["Cin"])
        else:
            x = x[:, :, :c["H"] * c["W"]].reshape(G, c["B"], c["H"], c["W"], c["Cin"])
        Arows = [_conv_rows(x, c, s, g) for g in range(G)]
    wcols = s.get("w_wrap") or K
    kreal = 9 * c["Cin"] if amode else K
    Wt = _rnd((G, N, wcols), seed + 2, scale=kreal ** -0.5)
    Wt[..., kreal:] = 0                                                           # W's K padding: zeros (the header's contract)
    Wt = Wt.half()
    wrows = N + (8 if pa else 0) if G > 1 else N
    Wbuf = torch.full((G * wrows + (32 if pa else 0), s["ldw"]), float("nan"), dtype=torch.half, device=dev)
    for g in range(G):
        Wbuf[g * wrows:g * wrows + N, :wcols] = Wt[g]
    kw["W"] = Wbuf
    Weff = Wt if not s.get("w_wrap") else torch.cat([Wt, Wt[..., :K - wcols]], -1)
    nbias = s["d2s_Co"] if epi == D2S else N                                      # D2S: bias[o], one per output channel
    nb = nbias + (8 if pa else 0) if G > 1 else nbias
    bias = _rnd((G, nbias), seed + 3)
    bbuf = torch.full((G * nb + 64,), float("nan"), device=dev)
    for g in range(G):
        bbuf[g * nb:g * nb + nbias] = bias[g]
    kw["bias"] = bbuf
    if epi == D2S:
        bias = bias.repeat(1, s["d2s_k"] ** 2)
    acc = [Arows[g] @ Weff[g].double().t() for g in range(G)]
    mag = [Arows[g].abs() @ Weff[g].double().abs().t() for g in range(G)]
    pre = [acc[g] + bias[g].double() for g in range(G)]
    pmag = [mag[g] + bias[g].double().abs() for g in range(G)]
    if c.get("lnin"):
        stats = torch.stack([_rnd((M,), seed + 7).abs() + 0.5, _rnd((M,), seed + 8) * 0.3], 1)
        wsum = Weff[0].float().sum(1)
        kw["row_stats_in"], kw["wsum"] = lg.poisoned(stats, post_rows=64), wsum
        pre = [stats[:, :1].double() * acc[0] + stats[:, 1:].double() * wsum.double() + bias[0].double()]
        pmag = [stats[:, :1].double() * mag[0] + (stats[:, 1:].double() * wsum.double()).abs() + bias[0].double().abs()]
    rows_in = s.get("rows_in", 0)
    if c.get("add"):
        nadd = (rows_in or M) + s.get("add_row_off", 0)
        addv = _rnd((nadd, N), seed + 4)
        kw["add"] = lg.poisoned(addv, ld=s["ldadd"], post_rows=32)
        ar = (torch.arange(M, device=dev) % rows_in if rows_in else torch.arange(M, device=dev)) + s.get("add_row_off", 0)
        pre = [p + addv[ar].double() for p in pre]
        pmag = [p + addv[ar].double().abs() for p in pmag]
    m = torch.arange(M, device=dev)
    ck = (m % s["rows_img"] < c["H"] * c["W"]) if amode else torch.ones(M, dtype=torch.bool, device=dev)
    orow = (m // rows_in) * s["rows_out"] + m % rows_in + s["row_off"] if rows_in else m
    if c.get("splitk"):
        nws = s["splitk_ws_bytes"] // 4 if c["splitk"] == 2 else 256 * 16384
        kw["splitk_ws"] = torch.empty(nws, device=dev)
        kw["splitk_cnt"] = torch.zeros(2048, dtype=torch.int32, device=dev)
    outs, checks, gs = {}, [], []
    tile = (128, 128)
    if epi in (F16, F32):
        dt = torch.half if epi == F16 else torch.float32
        gap = c.get("gap", 0) * pc
        per = s["gOut"] // s["ldc"] if G > 1 else (int(orow.max()) + 1 + (s["rows_out"] - s["rows_in"] - s["row_off"] if rows_in else 0))
        R = per * G - (gap if G > 1 else 0)
        valid = torch.cat([orow + g * per for g in range(G)])
        init = None
        if epi == F32 and s["accumulate"]:                                        # the same old values on the written rows at every layout
            init = torch.zeros(R, N, device=dev)
            init[valid] = _rnd((valid.numel(), N), seed + 5)
        go = lg.guarded(R, N, s["ldc"], dt, offset_cols=(8 if dt == torch.half else 4) if pc else 0, rows_inside=valid, init=init)
        if init is not None:
            init = go.view.clone()
        kw["out"] = go.view
        gs.append(go)
        old = [init[orow + g * per].double() if init is not None and s["accumulate"] else 0.0 for g in range(G)]
        res = [pre[g] + old[g] for g in range(G)]
        rmag = [pmag[g] + (old[g].abs() if init is not None and s["accumulate"] else 0.0) for g in range(G)]
        stored = [_act(r, s["act"]) for r in res]
        if epi == F32 and s["accumulate"] == 2:
            checks.append(("same", "out untouched (accumulate 2)", go.view, init))
        else:
            for g in range(G):
                checks.append(("ew", "out", go.view, valid[g * M:(g + 1) * M][ck], stored[g][ck], rmag[g][ck], dt == torch.half, s["act"] == GELU))
        if "out2" in ptrs:
            go2 = lg.guarded(R, N, s["ldc2"], torch.half, offset_cols=8 if pc else 0, rows_inside=valid)
            kw["out2"] = go2.view
            gs.append(go2)
            for g in range(G):
                checks.append(("ew", "out2", go2.view, valid[g * M:(g + 1) * M][ck], _act(stored[g], s["act2"])[ck], rmag[g][ck], True,
                               s["act"] == GELU or s["act2"] == GELU))
        if c.get("maxo"):
            mo_init = _rnd((R, N), seed + 6)
            gm = lg.guarded(R, N, s["ldc"], torch.float32, offset_cols=4 if pc else 0, init=mo_init)
            kw["max_out"] = gm.view
            gs.append(gm)
            checks.append(("max", "max_out", gm, mo_init, go))
        if c.get("rso"):
            slabs = N // 64
            grs = lg.guarded(M, 2 * slabs, 2 * slabs, torch.float32)
            kw["row_stats_out"] = grs.view
            gs.append(grs)
            checks.append(("rso", "row_stats_out", grs, go))
            if c.get("rsf"):
                grf = lg.guarded(M, 2, 2, torch.float32)
                kw["row_stats_final"], kw["row_stats_ticket"] = grf.view, torch.zeros(-(-M // 128) + 64, dtype=torch.int32, device=dev)
                gs.append(grf)
                checks.append(("rsf", "row_stats_final", grf, go))
    elif epi == QKV:
        D2, B, H = s["vsplit"], c["B"], c["heads"]
        T = s["tok_per_img"]
        R = M * G
        gq = lg.guarded(R, D2, s["ldc"], torch.half, offset_cols=8 if pc else 0)
        vt_rows = B * H * 64
        gv = lg.guarded(G * vt_rows, s["kv_ld"], s["kv_ld"], torch.half, init=torch.zeros(G * vt_rows, s["kv_ld"], device=dev).half())
        kw["out"], kw["out2"] = gq.view, gv.view
        gs += [gq, gv]
        vc = _vcols(T).cuda()
        gv.cmp = lambda: gv.view.view(G * B * H * 64, -1)[:, vc]                  # the key columns (kv_ld differs between layouts)
        for g in range(G):
            act_pre = _act(pre[g], s["act"])
            checks.append(("ew", "q|k", gq.view, m + g * M, act_pre[:, :D2], pmag[g][:, :D2], True, s["act"] == GELU))
            want = act_pre[:, D2:].reshape(B, T, H, 64).permute(0, 2, 3, 1)
            wmag = pmag[g][:, D2:].reshape(B, T, H, 64).permute(0, 2, 3, 1)
            checks.append(("vt", "V^T", gv.view[g * vt_rows:(g + 1) * vt_rows].view(B, H, 64, s["kv_ld"]), vc, want, wmag))
    elif epi == D2S:
        k, Co, B = s["d2s_k"], s["d2s_Co"], c["B"]
        Hin, Win, opix = s["d2s_Hin"], s["d2s_Win"], s["d2s_out_img_pix"]
        Ho, Wo = Hin * k, Win * k
        R = B * opix
        valid = torch.cat([b * opix + torch.arange(Ho * Wo, device=dev) for b in range(B)])
        init = torch.zeros(R, Co, device=dev)
        init[valid] = _rnd((valid.numel(), Co), seed + 5)
        go = lg.guarded(R, Co, s["ldc"], torch.float32, offset_cols=4 if pc else 0, rows_inside=valid, init=init)
        init = go.view.clone()
        kw["out"] = go.view
        gs.append(go)
        rin = s["d2s_rows_in_img"]
        pr = pre[0].view(B, rin, N)[:, :Hin * Win].reshape(B, Hin, Win, k, k, Co).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho * Wo, Co)
        mg = pmag[0].view(B, rin, N)[:, :Hin * Win].reshape(B, Hin, Win, k, k, Co).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho * Wo, Co)
        res = init[valid].view(B, Ho * Wo, Co).double() + pr
        rmag = init[valid].view(B, Ho * Wo, Co).double().abs() + mg
        checks.append(("ew", "out", go.view, valid, res.reshape(-1, Co), rmag.reshape(-1, Co), False, False))
        if "out2" in ptrs:
            go2 = lg.guarded(R, Co, s["ldc2"], torch.half, offset_cols=8 if pc else 0, rows_inside=valid)
            kw["out2"] = go2.view
            gs.append(go2)
            checks.append(("ew", "out2", go2.view, valid, _act(res, s["act2"]).reshape(-1, Co), rmag.reshape(-1, Co), True, False))
    else:                                                                         # HEAD
        w2 = _rnd((G, 32), seed + 9, scale=0.2)
        w2buf = torch.full((G * s.get("gW2", 32) + 32,), float("nan"), device=dev)
        for g in range(G):
            w2buf[g * s.get("gW2", 32):g * s.get("gW2", 32) + 32] = w2[g]
        kw["w2"] = w2buf
        go = lg.guarded(G, M, s["gOut"], torch.float32, offset_cols=4 if pc else 0)
        kw["out"] = go.view
        gs.append(go)
        for g in range(G):
            h = _act(pre[g], LRELU)
            y = h @ w2[g].double() + (s["b2"] if g == 0 else s["b2_g1"])
            o = torch.exp(y.clamp(-8, 8) + (s["post_add"] if g == 0 else s["post_add_g1"]))
            ymag = pmag[g] @ w2[g].double().abs()
            r_mag = 2.0 ** -11 if amode == 3 else 0.0                             # the kernel rounds the interpolated A operand to fp16
            checks.append(("head", "HEAD", go.view[g], o, o * ymag, o * (16 * 2.0 ** -24) * (1 + y.abs()), r_mag))
    # ---- launch
    d = ops.mk(ops.UdGemm, **kw)
    assert ops.lib.ud_gemm_pick(C.byref(d)) == c["pick"], (c["id"], lay, ops.lib.ud_gemm_pick(C.byref(d)))
    ops.gemm(**kw)
    torch.cuda.synchronize()
    # ---- checks
    tag = f"{c['id']} {lay}"
    worst = 0.0
    for kind, name, *a in checks:
        if kind == "same":
            assert torch.equal(_bits(a[0]), _bits(a[1])), f"{tag}: {name}"
        elif kind == "vt":
            vt, vc, want, wmag = a
            worst = max(worst, lg.assert_elementwise(vt[..., vc].reshape(-1, vc.numel()), want.reshape(-1, vc.numel()), wmag.reshape(-1, vc.numel()), K,
                                                     fp16_out=True, gelu=s["act"] == GELU, name=f"{tag} {name}"))
            unused = torch.ones(vt.shape[-1], dtype=torch.bool, device=dev)
            unused[vc] = False
            assert bool((_bits(vt[..., unused]) == 0).all()), f"{tag}: V^T columns outside the key map must stay zero"
        elif kind == "head":
            ov, o, omag, atol, r_mag = a
            worst = max(worst, lg.assert_elementwise(ov, o, omag, K, r_mag=r_mag, atol=atol, name=f"{tag} {name}"))
        elif kind == "max":
            gm, mo_init, go = a
            assert torch.equal(_bits(gm.view), _bits(torch.maximum(mo_init, go.view))), f"{tag}: {name}"
        elif kind == "rso":
            grs, go = a
            x = go.view[orow].double().view(M, -1, 64)
            want = torch.stack([x.sum(-1), (x * x).sum(-1)], -1).view(M, -1)
            wmag = torch.stack([x.abs().sum(-1), (x * x).sum(-1)], -1).view(M, -1)
            worst = max(worst, lg.assert_elementwise(grs.view, want, wmag, 64, name=f"{tag} {name}"))
        elif kind == "rsf":
            grf, go = a
            x = go.view[orow].double()
            mean, var = x.mean(1), x.var(1, unbiased=False)
            rstd = 1.0 / torch.sqrt(var + 1e-6)
            want = torch.stack([rstd, -mean * rstd], 1)
            wmag = torch.stack([rstd, (x.abs().mean(1) + x.std(1)) * rstd], 1)
            worst = max(worst, lg.assert_elementwise(grf.view, want, wmag, N * N, name=f"{tag} {name}"))
        else:
            view, rows, ref, mg, f16, gelu = a
            worst = max(worst, lg.assert_elementwise(view[rows], ref, mg, K, fp16_out=f16, gelu=gelu, tile=tile, name=f"{tag} {name}"))
    print(f"RATIO gemm {c['id']} {'strided' if lay != (0, 0) else 'dense'}{lay} {worst:.4f}")          # the worst error / bound over the case's outputs
    for i, g in enumerate(gs):
        g.check_guards(f"{c['id']} {lay} output {i}")
    return [g.written() if not hasattr(g, "cmp") else g.cmp() for g in gs]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c["id"] for c in GEMM_CASES])
def test_gemm_layouts(ops, case):
    """Every schedule of ud_gemm_f16 at the product's layout and at strided / offset / guarded layouts: each element inside the fp64 bound,
    every guard element intact, and the strided results bit-identical to the first layout's."""
    ref = None
    for lay in _lay(case):
        got = run_gemm(ops, case, lay)
        if ref is None:
            ref = got
        else:
            for i, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{case['id']}: output {i} at layout {lay} differs from {_lay(case)[0]}"


# ---- linear_f32 (the camera adapter's interleaved slices) ------------------------------------------------------------------------------
LINEAR_CASES = [dict(M=M, N=N, K=K, xpad=xp, cpad=cp, add=ad, act=act, acc=acc) for (M, N, K, act, acc) in ((4, 512, 512, GELU, 0), (37, 60, 256, 0, 1))
                for xp, cp, ad in sorted(LINEAR_F32_FLAGS)]


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "M{M}N{N}K{K}_x{xpad:d}c{cpad:d}add{add:d}".format(**c))
def test_linear_f32_interleaved_slices(ops, case):
    """ud_linear_f32 writing the four interleaved column slices of one buffer (ldc = 4 N, + a guarded gap with cpad) by four calls, as the
    camera adapter does: each slice inside the fp32 bound, the neighbours' columns untouched until their own call (bitwise)."""
    M, N, K = case["M"], case["N"], case["K"]
    ldx = K + (68 if case["xpad"] else 0)
    ldc = (4 * N + 256) if case["cpad"] else N        # cpad = 0: the plain dense layout, one slice
    slices = 4 if case["cpad"] else 1
    off = 4 if case["cpad"] else 0
    init = _rnd((M, ldc - off), 11) if case["acc"] else None
    go = lg.guarded(M, ldc - off, ldc, torch.float32, offset_cols=off, rows_inside=torch.arange(M, device="cuda"), init=init)
    go.inside[:] = False                               # nothing may be written before the first call
    before = go.buf.clone()
    for j in range(slices):
        x = lg.poisoned(_rnd((M, K), 20 + j), ld=ldx, post_rows=8)
        W = lg.poisoned(_rnd((N, K), 30 + j, scale=K ** -0.5), ld=K, post_rows=8)
        b = _rnd((N,), 40 + j)
        kw = dict(x=x, W=W, bias=b, M=M, N=N, K=K, ldx=ldx, ldw=K, ldc=ldc, act=case["act"], accumulate=case["acc"])
        pre = x.double() @ W.double().t() + b.double()
        mag = x.double().abs() @ W.double().abs().t() + b.double().abs()
        if case["add"]:
            am = 4
            a = lg.poisoned(_rnd((am, N), 50 + j), ld=N + 64)
            kw.update(add=a, ldadd=N + 64, add_mod=am)
            ar = torch.arange(M, device="cuda") % am
            pre, mag = pre + a[ar].double(), mag + a[ar].double().abs()
        view = go.buf[go.pre:go.pre + M, off + j * N:off + (j + 1) * N]
        old = view.double().clone() if case["acc"] else 0.0
        mag = mag + (old.abs() if case["acc"] else 0.0)
        ref = _act(pre, case["act"]) + old if case["acc"] else _act(pre, case["act"])
        d = ops.mk(ops.UdLinearF32, out=view, **kw)
        ops.check(ops.lib.ud_linear_f32(C.byref(d), ops.cur_stream()), "ud_linear_f32")
        torch.cuda.synchronize()
        lg.assert_elementwise(view, ref, mag, K, gelu=case["act"] == GELU, name=f"slice {j}")
        go.inside[go.pre:go.pre + M, off + j * N:off + (j + 1) * N] = True
        bits, b0 = _bits(go.buf), _bits(before)
        assert torch.equal(bits[~go.inside], b0[~go.inside]), f"slice {j}: a write outside the slice"


# ---- attention -------------------------------------------------------------------------------------------------------------------------
# layout: 0 dense (ld = H*64, rows = Nq / Nk), 1 packed like the product ([q | k] rows of ld 2 H*64, O dense), 2 strided (every ld padded)
ATT_CASES = [dict(B=B, H=H, Nq=Nq, Nk=Nk, lay=lo, pad=pad, bc=bc, pre=pre) for (B, H, Nq, Nk) in ((2, 3, 200, 77), (24, 8, 300, 300))
             for lo in (0, 1, 2) for pad in (0, 1) for bc in (0, 1) for pre in (0, 1)]
ATT_CASES += [dict(B=9, H=16, Nq=1370, Nk=1370, lay=2, pad=1, bc=0, pre=1), dict(B=40, H=8, Nq=200, Nk=200, lay=1, pad=1, bc=1, pre=0)]


def attention_case_flags(c):
    lo = c["lay"]
    return (lo >= 1, lo >= 1, lo == 2, bool(c["pad"]), bool(c["bc"]), bool(c["pre"]))


@pytest.mark.parametrize("c", ATT_CASES, ids=lambda c: "B{B}H{H}N{Nq}x{Nk}_lay{lay}pad{pad}bc{bc}pre{pre}".format(**c))
def test_attention_layouts(ops, c):
    """ud_attention_f16 with poisoned stride gaps, poisoned token rows past Nq / Nk, poisoned V^T columns past the 64-aligned key count, kv
    broadcast (groups of 2 images per K/V image) and pre-scaled Q: every output element inside the bound, padding rows and gaps of O intact."""
    B, H, Nq, Nk, lo = c["B"], c["H"], c["Nq"], c["Nk"], c["lay"]
    D = H * 64
    qr, kr = (Nq + 8 if c["pad"] else Nq), (Nk + 5 if c["pad"] else Nk)
    kv64 = (Nk + 63) // 64 * 64
    kv_ld = kv64 + (64 if lo == 2 else 0)
    grp = 2 if c["bc"] else 1
    Bk = -(-B // grp)
    ldq = ldk = D if lo == 0 else 2 * D + (64 if lo == 2 else 0)
    ldo = D + (128 if lo == 2 else 0)
    q = _rnd((B, qr, D), 1).half()
    k = _rnd((Bk, kr, D), 2).half()
    v = _rnd((Bk, Nk, D), 3).half()
    q[:, Nq:] = float("nan")
    k[:, Nk:] = float("nan")
    scale = 0.125
    qin = (q.double() * scale * math.log2(math.e)).half() if c["pre"] else q
    if lo == 0:
        Q, K = lg.poisoned(qin.reshape(-1, D), post_rows=8), lg.poisoned(k.reshape(-1, D), post_rows=8)
    else:
        qk = torch.full((max(B * qr, Bk * kr) + 8, ldq), float("nan"), dtype=torch.half, device="cuda")
        qk[:B * qr, :D] = qin.reshape(-1, D)
        kb = torch.full_like(qk, float("nan"))                                      # K in its own [.. | k] rows (Bk <= B images)
        kb[:Bk * kr, D:2 * D] = k.reshape(-1, D)
        Q, K = qk[:, :D], kb[:, D:2 * D]
    vt = torch.zeros(Bk, H, 64, kv_ld, dtype=torch.half, device="cuda")
    vt[..., kv64:] = float("nan")                                             # past the zero padding the header requires: poison
    vt[..., _vcols(Nk).cuda()] = v.view(Bk, Nk, H, 64).permute(0, 2, 3, 1)
    go = lg.guarded(B * qr, D, ldo, torch.half, offset_cols=8 if lo == 2 else 0,
                    rows_inside=torch.cat([b * qr + torch.arange(Nq) for b in range(B)]).cuda())
    ops.attention(Q=Q, K=K, Vt=vt, O=go.view, B=B, H=H, Nq=Nq, Nk=Nk, ldq=ldq, ldk=ldk, ldo=ldo, kv_ld=kv_ld, q_rows_per_img=qr,
                  k_rows_per_img=kr, scale=scale, kv_broadcast=c["bc"], kv_group=grp if c["bc"] else 0, q_prescaled=c["pre"])
    torch.cuda.synchronize()
    for b in range(B):
        kb_ = b // grp
        qf = qin[b, :Nq].double().view(Nq, H, 64).transpose(0, 1)
        kf = k[kb_, :Nk].double().view(Nk, H, 64).transpose(0, 1)
        vf = v[kb_].double().view(Nk, H, 64).transpose(0, 1)
        s = qf @ kf.transpose(-1, -2)
        p = torch.softmax(s * (math.log(2.0) if c["pre"] else scale), -1)
        ref = (p @ vf).transpose(0, 1).reshape(Nq, D)
        mag = (p @ vf.abs()).transpose(0, 1).reshape(Nq, D)
        lg.assert_elementwise(go.view[b * qr:b * qr + Nq], ref, mag, 64, fp16_out=True, r_mag=2.0 ** -10, tile=(64, 64), name=f"image {b}")
    go.check_guards("O")


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [384, 1024])
@pytest.mark.parametrize("flags", sorted(LAYERNORM_FLAGS), ids=lambda f: "x{:d}y{:d}remap{:d}cls{:d}f32{:d}add{:d}".format(*f))
def test_layernorm_layouts(ops, flags, D):
    """ud_layernorm_f32_f16 at ldx / ldy > D (poisoned input gaps, guarded output gaps), the row remap of the encoder taps, the class-token
    side output cls_y (ldcls > D), fp32 output and the `add` input: every element inside the bound, every guard element intact."""
    xpad, ypad, remap, cls, f32, add = flags
    B, n = 3, 19
    rin, rout, ioff, ooff = (24, 26, 2, 3) if remap else (n + cls, n, int(cls), 0)      # cls_y: the class-token row in front of the tokens
    ldx, ldy = D + (64 if xpad else 0), D + (256 if ypad else 0)
    x = _rnd((B * rin, D), 1) * 3 + 0.7
    x.view(B, rin, D)[:, ioff + n:] = float("nan")                             # rows past an image's tokens: poison
    if ioff > (1 if cls else 0):
        x.view(B, rin, D)[:, :ioff - (1 if cls else 0)] = float("nan")
    X = lg.poisoned(x, ld=ldx, post_rows=4)
    odt = torch.float32 if f32 else torch.half
    orows = torch.cat([b * rout + ooff + torch.arange(n) for b in range(B)]).cuda()
    go = lg.guarded(B * rout, D, ldy, odt, offset_cols=(8 if ypad else 0), rows_inside=orows)
    kw = dict(x=X, y=go.view, rows=B * (n + (1 if cls else 0)), D=D, ldx=ldx, ldy=ldy, eps=1e-6, rows_per_img=n, in_rows_per_img=rin, in_row_off=ioff,
              out_rows_per_img=rout, out_row_off=ooff, out_f32=int(f32))
    xin = x.view(B, rin, D)[:, ioff:ioff + n].double()
    if add:
        a = _rnd((rout + 2, D), 5)
        kw["add"] = lg.poisoned(a, ld=ldx)
        xin = xin + a[ooff:ooff + n].double()
    gc = None
    if cls:
        ldcls = D + (64 if ypad else 0)
        gc = lg.guarded(B, D, ldcls, torch.float32, offset_cols=4 if ypad else 0)
        kw.update(cls_y=gc.view, ldcls=ldcls)
    ops.layernorm(**kw)
    torch.cuda.synchronize()
    ref = F.layer_norm(xin, (D,), eps=1e-6)
    lg.assert_elementwise(go.view[orows], ref.reshape(-1, D), ref.abs().reshape(-1, D) + 1.0, D, fp16_out=not f32, name="y")
    go.check_guards("y")
    if cls:
        cref = F.layer_norm(x.view(B, rin, D)[:, ioff - 1].double(), (D,), eps=1e-6)
        lg.assert_elementwise(gc.view, cref, cref.abs() + 1.0, D, name="cls_y")
        gc.check_guards("cls_y")


# ---- preprocess_patches: pad columns untouched -----------------------------------------------------------------------------------------
def test_preprocess_patches_leaves_pad_columns_untouched(ops):
    """include/unidepth_hip.h UdPreprocess: row stride ldp >= 588, "pad cols untouched" -- checked on a sentinel-filled buffer (the suite's
    own test starts from zeros, so a zero written into the pad could not be seen)."""
    B, H, W, pl, pr, pt, pb, Hn, Wn = 2, 30, 50, 0, 0, 3, 4, 28, 42
    Hp, Wp = H + pt + pb, W + pl + pr
    g = torch.Generator().manual_seed(0)
    rgb = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    hw = (Hn // 14) * (Wn // 14)
    ldp = 588 + 260
    go = lg.guarded(B * hw, 588, ldp, torch.half, offset_cols=8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    d = ops.mk(ops.UdPreprocess, rgb=rgb, patches=go.view, B=B, H=H, W=W, pad_l=pl, pad_t=pt, Hp=Hp, Wp=Wp, Hn=Hn, Wn=Wn,
               ldp=ldp, is_u8=1, normalize=1, mean=mean, inv_std=tuple(1.0 / s for s in std))
    ops.check(ops.lib.ud_preprocess_patches(C.byref(d), ops.cur_stream()))
    x = rgb.double() / 255.0
    x = (x - torch.tensor(mean, device="cuda", dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, device="cuda", dtype=torch.float64).view(1, 3, 1, 1)
    x = F.interpolate(F.pad(x, (pl, pr, pt, pb)), size=(Hn, Wn), mode="bilinear", align_corners=False)
    ref = F.unfold(x, kernel_size=14, stride=14).transpose(1, 2).reshape(B * hw, 588)
    torch.cuda.synchronize()
    lg.assert_elementwise(go.view, ref, ref.abs() + 4.0, 64, fp16_out=True, name="patches")
    go.check_guards("patches")


ATTENTION_FLAGS = {attention_case_flags(c) for c in ATT_CASES}
_spec = importlib.util.spec_from_file_location("test_attention_paths_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_attention_paths_gpu.py"))
att_paths = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(att_paths)
ATTENTION_SCHEDULES = {_attention_schedule(c["B"], c["H"], c["Nq"], c["Nk"], bool(c["pre"])) for c in ATT_CASES + att_paths.CASES}
