"""ud_knn_points (csrc/evalops.hip) at every kernel class its dispatch can take -- knn1_d3_kernel<L2> and knn_kernel<DC, KT>, unsplit and
split over P2 -- against the numpy restatement of the reference's CPU K-NN (oracle/restate_eval.py), bit for bit in distances and
indices.  The cases and the class each one reaches are tests/knn_cases.py (checked on the host by tests/test_knn_paths_cpu.py): ragged
lengths on both sides, exact ties across chunks, tiles and slices, distances that are all +inf, guarded outputs and work area, inputs
behind a NaN head, a dirty work area, lengths outside [0, P], and the wrapper's return_nn.  The descriptor is driven directly."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import knn_cases as kc
import layout_guard as lg
from oracle import restate_eval as re_

pytestmark = pytest.mark.gpu

ISENT = 0x5A5A5A5A
IDS = [c["id"] for c in kc.CASES]
HEAD = 63


def _int_guarded(n, dtype, pad=64):
    buf = torch.full((pad + n + pad,), ISENT, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + n], pad


def _int_guard_intact(buf, n, pad):
    return bool((buf[:pad] == ISENT).all()) and bool((buf[pad + n:] == ISENT).all())


def _nan_headed(t):
    """t as the exact-size tail of an allocation whose head holds quiet NaN (and leaves the data 4-byte aligned only, which is all the
    C-ABI asks): a read before the start of an input lands on NaN."""
    buf = lg._filled(HEAD + t.numel(), torch.float32, lg.QNAN[torch.float32], "cuda")
    buf[HEAD:] = t.reshape(-1).cuda()
    return buf, buf[HEAD:]


def _launch(case, p1, p2, l1, l2, dists, idx, work):
    from unidepth_amd import _lib
    from unidepth_amd.ops import cur_stream, mk
    d = mk(_lib.UdKnn, p1=p1, p2=p2, lengths1=l1, lengths2=l2, dists=dists, idx=idx, work=work, N=kc.N, P1=case["P1"], P2=case["P2"],
           D=case["D"], K=case["K"], norm=case["norm"])
    assert (int(_lib.lib.ud_knn_split(C.byref(d))) > 1) == case["split"]
    _lib.check(_lib.lib.ud_knn_points(C.byref(d), cur_stream()), "ud_knn_points")
    torch.cuda.synchronize()


def _plain(case, l1, l2, work_byte=0x00):
    """(dists, idx) as numpy from dense buffers; outputs start as NaN / -1 (every element must be written), work as `work_byte`."""
    p1, p2 = kc.inputs(case)
    n = kc.N * case["P1"]
    dists = torch.full((n * case["K"],), float("nan"), device="cuda")
    idx = torch.full((n * case["K"],), -1, dtype=torch.int64, device="cuda")
    work = torch.full((n * 8,), work_byte, dtype=torch.uint8, device="cuda") if case["split"] else None
    _launch(case, p1.cuda(), p2.cuda(), l1.cuda(), l2.cuda(), dists, idx, work)
    shape = (kc.N, case["P1"], case["K"])
    return dists.cpu().numpy().reshape(shape), idx.cpu().numpy().reshape(shape)


@functools.lru_cache(maxsize=None)
def _gpu(id, variant="full"):
    return _plain(kc.BY_ID[id], *kc.lengths(kc.BY_ID[id], variant))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_same(case, got, ref, what):
    (d, i), (rd, ri) = got, ref
    bad = np.argwhere(_bits(d) != _bits(rd))
    assert bad.size == 0, (f"{case['id']} {what}: {len(bad)} distance(s) differ; first at (n, q, k) = {tuple(bad[0])}: "
                           f"{d[tuple(bad[0])]!r} vs {rd[tuple(bad[0])]!r}")
    # a slot whose distance is +inf was never a candidate of the register list: its index is 0 (include/unidepth_hip.h), where the
    # restatement's stable sort numbers such slots 0, 1, 2, ..; for K = 1 both are 0 and the comparison is complete
    keep = np.isfinite(rd) if case["K"] > 1 else np.ones(rd.shape, bool)
    bad = np.argwhere((i != ri) & keep)
    assert bad.size == 0, (f"{case['id']} {what}: {len(bad)} index/indices differ; first at (n, q, k) = {tuple(bad[0])}: "
                           f"{i[tuple(bad[0])]} vs {ri[tuple(bad[0])]}")
    assert (i[~keep] == 0).all(), f"{case['id']} {what}: an index of a +inf slot is not 0"


@pytest.mark.parametrize("variant", kc.VARIANTS)
@pytest.mark.parametrize("case", kc.CASES, ids=IDS)
def test_matches_restatement_bit_for_bit(case, variant):
    _assert_same(case, _gpu(case["id"], variant), kc.reference(case, variant), variant)


@pytest.mark.parametrize("variant", kc.VARIANTS)
@pytest.mark.parametrize("id", [c["id"] for c in kc.CASES if c["data"] == "overflow"])
def test_all_inf_distances_give_inf_and_index_zero(id, variant):
    """a query with an inf coordinate, and one whose squared distances overflow, are at distance +inf from everything: dists = +inf and
    idx = 0 in every filled slot, split or not -- never the distance 0 of a padding slot, which the metrics would count as a match"""
    case = kc.BY_ID[id]
    d, i = _gpu(id, variant)
    l1, l2 = (v.tolist() for v in kc.lengths(case, variant))
    seen = 0
    for n in range(kc.N):
        if l1[n] == 0 or l2[n] == 0:
            continue
        kv = min(case["K"], l2[n])
        for q in kc.OVERFLOW_ROWS:
            print(id, variant, "cloud", n, "query", q, "dists", d[n, q], "idx", i[n, q])
            assert np.isposinf(d[n, q, :kv]).all() and (i[n, q] == 0).all(), (n, q, d[n, q], i[n, q])
            assert (d[n, q, kv:] == 0).all()
            seen += 1
    assert seen == 2


@pytest.mark.parametrize("id", kc.GUARDED)
def test_outputs_and_work_area_stay_inside_their_allocations(id):
    case = kc.BY_ID[id]
    p1, p2 = kc.inputs(case)
    l1, l2 = kc.lengths(case)
    n = kc.N * case["P1"]
    nk = n * case["K"]
    dg = lg.guarded(1, nk, nk + 5, torch.float32, pre_rows=2, post_rows=2, offset_cols=3)
    ibuf, idx, ipad = _int_guarded(nk, torch.int64)
    wbuf, work, wpad = _int_guarded(n, torch.int64)
    b1, v1 = _nan_headed(p1)
    b2, v2 = _nan_headed(p2)
    _launch(case, v1, v2, l1.cuda(), l2.cuda(), dg.ptr(), idx, work if case["split"] else None)
    dg.check_guards("dists")
    assert _int_guard_intact(ibuf, nk, ipad), "idx: guard rewritten"
    assert _int_guard_intact(wbuf, n, wpad), "work: guard rewritten"
    if not case["split"]:
        assert bool((work == ISENT).all()), "work: written without being passed"
    ref = _gpu(id)
    shape = ref[0].shape
    assert np.array_equal(_bits(dg.view.cpu().numpy().reshape(shape)), _bits(ref[0]))
    assert np.array_equal(idx.cpu().numpy().reshape(shape), ref[1])
    qnan = lg.QNAN[torch.float32]
    assert bool((b1[:HEAD].view(torch.int32) == qnan).all()) and bool((b2[:HEAD].view(torch.int32) == qnan).all())      # inputs are read-only
    assert np.array_equal(v1.cpu().numpy(), p1.reshape(-1).numpy()) and np.array_equal(v2.cpu().numpy(), p2.reshape(-1).numpy())


@pytest.mark.parametrize("variant", kc.VARIANTS)
@pytest.mark.parametrize("id", [c["id"] for c in kc.CASES if c["split"] and c["data"] in ("randn", "overflow")])
def test_split_result_does_not_depend_on_what_the_work_area_held(id, variant):
    case = kc.BY_ID[id]
    ref = _gpu(id, variant)                                     # work pre-filled with 0x00
    d, i = _plain(case, *kc.lengths(case, variant), work_byte=0xA5)
    assert np.array_equal(_bits(d), _bits(ref[0])) and np.array_equal(i, ref[1])


@pytest.mark.parametrize("id", ["fast1_l2", "knn_d4_k4_l1", "fast1_l1_split", "knn_d9_k1_l2_split"])
def test_lengths_outside_the_cloud_clamp(id):
    """lengths above P and below 0 act as P and 0"""
    case = kc.BY_ID[id]
    P1, P2 = case["P1"], case["P2"]
    wild = (torch.tensor([P1 + 7, -3, 2 ** 40]), torch.tensor([2 ** 40, P2 + 100, -1]))
    tame = (torch.tensor([P1, 0, P1]), torch.tensor([P2, P2, 0]))
    p1, p2 = kc.inputs(case)
    ref = re_.knn_points(p1.numpy(), p2.numpy(), tame[0].numpy(), tame[1].numpy(), case["norm"], case["K"])
    _assert_same(case, _plain(case, *wild), ref, "wild lengths")
    _assert_same(case, _plain(case, *tame), ref, "clamped lengths")


@pytest.mark.parametrize("id", ["knn_d3_k8_l2", "knn_d8_k2_l1", "fast1_l2_split"])
def test_wrapper_return_nn_equals_gather(id):
    from unidepth_amd import eval_ops
    case = kc.BY_ID[id]
    p1, p2 = kc.inputs(case)
    for variant in kc.VARIANTS:
        l1, l2 = kc.lengths(case, variant)
        rd, ri = kc.reference(case, variant)
        r = eval_ops.knn_points(p1.cuda(), p2.cuda(), l1.cuda(), l2.cuda(), norm=case["norm"], K=case["K"], return_nn=True)
        _assert_same(case, (r.dists.cpu().numpy(), r.idx.cpu().numpy()), (rd, ri), f"wrapper {variant}")
        assert np.array_equal(_bits(r.knn.cpu().numpy()), _bits(re_.knn_gather(p2.numpy(), ri, l2.numpy())))
