"""The K-NN cases of tests/test_knn_paths_gpu.py, shared with tests/test_knn_paths_cpu.py (not a conftest: the test modules import it).

ud_knn_points (csrc/evalops.hip) dispatches on (K, D, norm, work) to 30 kernel classes: knn1_d3_kernel<L2> (K = 1, D <= 3; "fast1"),
knn_kernel<DC, KT> for DC in {3, 4, 8, 0} and KT in {1, 2, 4, 8, 16, 32}, and for K = 1 with a work area the same kernels with P2 split
over blockIdx.z.  CASES names every class at least once, at shapes chosen by the kernels' constants (256 / 512 queries per block, the
1024-point tile or the 256-point tile of DC = 0, the 8-point chunk of fast1, the slice span of a split); knn_class(case) computes the
class the dispatch takes, the split flag by the library's own host function ud_knn_split.  The CPU test fails by name when a class
loses its last case or a case stops reaching the class it declares.

Every case is N = 3 clouds with ragged lengths: lengths1 from {0, a value strictly inside the last query block, P1}, lengths2 from
{0, K - 1, P2}, paired so that no cloud is empty on both sides (lengths(): two such pairings per case).  K = 1 has no positive length
below K: its short length is 5 points (inside the first 8-point chunk), which also leaves the later slices of a split without a single
point to scan."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

N = 3
UNSPLIT_P1, UNSPLIT_P2 = 300, 1100         # second query block partly active; crosses the 1024 (256) tile, tail not a multiple of 8
FAST_P1 = 700                              # fast1: q1 = q0 + 256 straddles len1 in the second block
SPLIT_P2 = 4100                            # with N = 3: S = 3 slices of span 1367, not tile aligned
TIE_P2 = 2048 + 8


def _case(id, D, K, norm, P1, P2, split=False, data="randn"):
    return {"id": id, "D": D, "K": K, "norm": norm, "P1": P1, "P2": P2, "split": split, "data": data}


def _declare():
    cases = []
    # unsplit knn_kernel<DC, KT>: K equal to KT and strictly inside its bracket (3, 5, 12, 17), both norms, per DC
    for D, K, norm in [(1, 2, 2), (2, 3, 1), (3, 8, 2), (3, 12, 1), (2, 32, 2), (3, 17, 1),                 # DC = 3 (KT = 1 is fast1)
                       (4, 1, 1), (4, 2, 2), (4, 4, 1), (4, 5, 2), (4, 16, 1), (4, 17, 2),                  # DC = 4
                       (5, 1, 2), (8, 2, 1), (5, 3, 2), (8, 8, 1), (5, 12, 2), (8, 32, 1),                  # DC = 8
                       (9, 1, 1), (32, 2, 2), (9, 4, 1), (32, 5, 2), (9, 16, 1), (32, 17, 2)]:              # DC = 0
        cases.append(_case(f"knn_d{D}_k{K}_l{norm}", D, K, norm, UNSPLIT_P1, UNSPLIT_P2))
    # the packed K = 1, D <= 3 path
    for norm in (2, 1):
        cases.append(_case(f"fast1_l{norm}", 3, 1, norm, FAST_P1, UNSPLIT_P2))
        cases.append(_case(f"fast1_l{norm}_split", 3, 1, norm, FAST_P1, SPLIT_P2, split=True))
    cases.append(_case("fast1_d2_l2_split", 2, 1, 2, FAST_P1, SPLIT_P2, split=True))
    # knn_kernel<DC, 1> split over P2
    for D, norm in [(4, 2), (8, 1), (9, 2)]:
        cases.append(_case(f"knn_d{D}_k1_l{norm}_split", D, 1, norm, FAST_P1, SPLIT_P2, split=True))
    # exact ties: the lower index must win across 8-point chunks, 1024-point tiles and P2 slices
    for data in ("twin_half", "twin_next", "lattice"):
        for norm in (2, 1):
            cases.append(_case(f"ties_{data}_l{norm}", 3, 1, norm, FAST_P1, TIE_P2, data=data))
            cases.append(_case(f"ties_{data}_l{norm}_split", 3, 1, norm, FAST_P1, SPLIT_P2, split=True, data=data))
        cases.append(_case(f"ties_{data}_d4_k4", 4, 4, 2 if data != "twin_next" else 1, UNSPLIT_P1, TIE_P2, data=data))
    # distances that are all +inf: an inf coordinate, and a squared distance that overflows
    for D in (3, 4):
        cases.append(_case(f"overflow_d{D}_k1", D, 1, 2, FAST_P1, UNSPLIT_P2, data="overflow"))
        cases.append(_case(f"overflow_d{D}_k1_split", D, 1, 2, FAST_P1, SPLIT_P2, split=True, data="overflow"))
        cases.append(_case(f"overflow_d{D}_k4", D, 4, 2, UNSPLIT_P1, UNSPLIT_P2, data="overflow"))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


CASES = _declare()
BY_ID = {c["id"]: c for c in CASES}
OVERFLOW_ROWS = (0, 1)                     # the queries of an "overflow" case whose distances are all +inf

# one guarded C-ABI run per kernel family
GUARDED = ("fast1_l2", "fast1_l1_split", "knn_d3_k8_l2", "knn_d4_k5_l2", "knn_d8_k8_l1", "knn_d32_k17_l2", "knn_d8_k1_l1_split")

# the classes that must keep a case: 23 unsplit (DC, KT), 3 split (DC, 1), and fast1 for both norms, split and unsplit
REQUIRED_KNN = {(dc, kt, False) for dc in (3, 4, 8, 0) for kt in (1, 2, 4, 8, 16, 32) if (dc, kt) != (3, 1)} | {(dc, 1, True) for dc in (4, 8, 0)}
REQUIRED_FAST1 = {(norm, split) for norm in (1, 2) for split in (False, True)}


def queries_per_block(case):
    return 512 if case["K"] == 1 and case["D"] <= 3 else 256


VARIANTS = ("full", "short")


def lengths(case, variant="full"):
    """(lengths1, lengths2) int64 [3].  A pairing without a cloud that is empty on both sides leaves exactly one cloud with points on both,
    so every case runs under two pairings: "full" searches the whole p2 cloud, "short" a p2 cloud shorter than K; the searching p1 cloud is
    the full one or the one that ends inside the last query block, alternating with the case's position in the table, as does the
    order of the clouds."""
    P1, P2, K = case["P1"], case["P2"], case["K"]
    per = queries_per_block(case)
    start = (P1 - 1) // per * per
    mid = start + (P1 - start) // 2
    assert start < mid < P1
    short = K - 1 if K > 1 else 5
    pos = CASES.index(case)
    a, b = (P1, mid) if pos % 2 == 0 else (mid, P1)
    pairs = [(0, short), (b, 0), (a, P2)] if variant == "full" else [(0, P2), (a, 0), (b, short)]
    pairs = pairs[pos % 3:] + pairs[:pos % 3]
    return torch.tensor([p[0] for p in pairs], dtype=torch.int64), torch.tensor([p[1] for p in pairs], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _inputs(id):
    case = BY_ID[id]
    D, P1, P2, data = case["D"], case["P1"], case["P2"], case["data"]
    g = torch.Generator().manual_seed(7000 + CASES.index(case))
    if data == "lattice":                  # dozens of equal minima per query
        p1 = torch.randint(0, 4, (N, P1, D), generator=g).float()
        p2 = torch.randint(0, 4, (N, P2, D), generator=g).float()
    else:
        p1 = torch.randn(N, P1, D, generator=g)
        if data == "twin_half":            # every point has an exact twin half a cloud later: another tile, another slice
            base = torch.randn(N, P2 // 2, D, generator=g)
            p2 = torch.cat([base, base], 1)
        elif data == "twin_next":          # adjacent twins: (2i, 2i + 1) inside one 8-chunk up to point 512, then one single point, so
            base = torch.randn(N, P2 // 2, D, generator=g)       # that the later twins (2i - 1, 2i) sit across the 7|8 chunk borders
            rep = base.repeat_interleave(2, dim=1)               # and the 1023|1024 tile border
            p2 = torch.cat([rep[:, :512], torch.randn(N, 1, D, generator=g), rep[:, 512:P2 - 1]], 1)
        else:
            p2 = torch.randn(N, P2, D, generator=g)
    if data == "overflow":
        p1[:, OVERFLOW_ROWS[0], 0] = float("inf")                # inf - finite = inf
        p1[:, OVERFLOW_ROWS[1], :] = 3e19                        # (3e19 - x)^2 = 9e38 > FLT_MAX
    assert p2.shape == (N, P2, D)
    return p1.contiguous(), p2.contiguous()


def inputs(case):
    """(p1 [3,P1,D], p2 [3,P2,D]) on the CPU; built once and shared -- do not modify."""
    return _inputs(case["id"])


@functools.lru_cache(maxsize=None)
def _reference(id, variant):
    from oracle import restate_eval as re_
    case = BY_ID[id]
    p1, p2 = _inputs(id)
    l1, l2 = lengths(case, variant)
    with np.errstate(over="ignore", invalid="ignore"):
        return re_.knn_points(p1.numpy(), p2.numpy(), l1.numpy(), l2.numpy(), case["norm"], case["K"])


def reference(case, variant="full"):
    """(dists [3,P1,K] f32, idx [3,P1,K] i64) of oracle.restate_eval.knn_points; computed once and shared -- do not modify."""
    return _reference(case["id"], variant)


def host_desc(case, work=None):
    """The UdKnn of a case with null data pointers: enough for the host-only ud_knn_split, which reads K, work, P1, P2, D and N.  A case
    declared split carries a work area, here a dummy non-null address."""
    from unidepth_amd import _lib
    d = _lib.UdKnn()
    d.N, d.P1, d.P2, d.D, d.K, d.norm = N, case["P1"], case["P2"], case["D"], case["K"], case["norm"]
    d.work = (8 if case["split"] else None) if work is None else work
    return d


def knn_split(case):
    from unidepth_amd import _lib
    return int(_lib.lib.ud_knn_split(C.byref(host_desc(case))))


def knn_class(case):
    """("fast1" | "knn", DC, KT, norm, split) as ud_knn_points dispatches the case (the fast1 / DC choice of its launch sequence, the KT
    ladder of knn_launch_k), split = ud_knn_split(descriptor) > 1."""
    D, K = case["D"], case["K"]
    split = knn_split(case) > 1
    if K == 1 and D <= 3:
        return ("fast1", 3, 1, case["norm"], split)
    dc = 3 if D <= 3 else 4 if D == 4 else 8 if D <= 8 else 0
    kt = 1 if K == 1 else 2 if K == 2 else 4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32
    return ("knn", dc, kt, case["norm"], split)
