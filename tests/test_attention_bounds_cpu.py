"""The inputs and the bound of tests/test_attention_paths_gpu.py, checked on the CPU with no kernel (the style of
tests/test_pointwise_bounds_cpu.py).  restate() below is a plain torch statement of what the two attention kernels compute -- 64-key tiles,
fp32 scores, the deferred maximum with its per-32-row-wave `any` trigger and d = max(mt, 0), fp16 P, and for the pipelined form the offset
carried in the scores and the row sum over the ROUNDED P -- with the threshold as a parameter and the defects below as switches:

  A  clean, it stays inside HALF of the bound on every input set of the GPU module (one head of each), at threshold 7.9 and at 8.1 for the
     near-threshold cases: the bound does not fail a correct kernel;
  B  each planted defect leaves the bound on every case named for it: the inputs can see it.
       mask_long / mask_short   the key-tail mask one key long / short         every tile-count case with a tail
       no_o / no_l              O / the row sum not rescaled at a trigger       every rescale case
       vt_order                 V^T read without its [0, 2, 1, 3] block order   every case whose order moves a valid key (Nk > 4)
       next_tail                the rows after the last key arrive in place of the zero tail
     next_tail ALONE cannot reach the output of either kernel -- the mask overwrites whatever arrived, which the first half of its test
     states as bit-identity -- so it is planted the way it can: with the bound and the mask both taking the K buffer's row count for the
     key count, i.e. the first row past Nk is let through;
  C  predict_crossings() names exactly the (tile, wave) pairs in which the restatement rescales, every intended crossing lies >= 4 log2
     units above the threshold (3.9: a planted 12 is 12 up to the fp16 rounding of a shared key and, in the ramp, up to another wave's key
     of the same tile lifting the row's offset a little further) and every other pair >= 0.5 below -- fp32 moves a score by < 10^-4 -- and the rescale matrix triggers in every KIND x stage of body()."""
import importlib.util
import os

import pytest
import torch

_here = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("test_attention_paths_gpu", os.path.join(_here, "test_attention_paths_gpu.py"))
ap = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ap)
lg = ap.lg

KT, WAVE = ap.KT, ap.WAVE
CASES = ap.CASES
_cache = {}


def _probe(c):
    """One head of case `c`: q, k, v, the rows that follow its keys in the K buffer, cq, and (ref, bound) -- computed once, left unchanged."""
    if c["id"] not in _cache:
        x = ap.make_inputs(c)
        b, h = c["probe"]
        nxt = x["k"][b + 1, h] if b + 1 < c["B"] else torch.full((KT, 64), -4.0, dtype=torch.half)
        after = torch.cat([x["k_pad"][b, h], nxt, torch.full((KT, 64), -4.0, dtype=torch.half)])
        q, k, v = x["q"][b, h], x["k"][b, h], x["v"][b, h]
        ref, bound, _ = ap.attention_bound(q, k, v, x["cq"])
        _cache[c["id"]] = dict(q=q, k=k, v=v, after=after, cq=x["cq"], ref=ref, bound=bound, x=x)
    return _cache[c["id"]]


def restate(q, k, v, pre, thr=ap.THR, defect=None, after=None):
    """What the kernels compute for one head, in torch: pre = 1 the pipelined kernel (Q pre-scaled, the offset carried in the scores, row sum
    over the rounded P), pre = 0 the one-tile kernel on raw Q (P = exp2(fma(s, c, -m c)), row sum over the unrounded P).  `after`: the rows
    that arrive for the keys past Nk (None: zeros, the bounded descriptor).  Returns (O fp16 [Nq, 64], {(tile, wave)} rescaled, tile >= 1)."""
    Nq, Nk = q.shape[0], k.shape[0]
    nt, W = -(-Nk // KT), -(-Nq // WAVE)
    rows = torch.arange(W * WAVE).clamp(max=Nq - 1)                            # the rows past Nq are clamped copies of the last one
    qf = q.float()[rows]
    kp = torch.zeros(nt * KT, 64)
    kp[:Nk] = k.float()
    if after is not None:
        kp[Nk:] = after[:nt * KT - Nk].float()
    vp = torch.zeros(nt * KT, 64)                                              # V^T columns [Nk, 64 nt) are zero
    vp[:Nk] = v.float()
    if defect == "vt_order":
        vp = vp[lg.vt_cols(nt * KT)]
    n_valid = Nk + (defect in ("mask_long", "next_tail")) - (defect == "mask_short")
    tail = Nk % KT != 0
    S = qf @ kp.t()
    c = torch.tensor(ap.SCALE * ap.LOG2E, dtype=torch.float32)
    key = torch.arange(KT)
    m = torch.zeros(W * WAVE) if pre else torch.full((W * WAVE,), -1.0e30)
    l, o = torch.zeros(W * WAVE), torch.zeros(W * WAVE, 64)
    fired = set()
    for t in range(nt):
        s = S[:, KT * t:KT * (t + 1)].clone()
        if pre:
            s = s - m[:, None]
        if t == nt - 1 and tail:
            s[:, KT * t + key >= n_valid] = -1.0e30
        mt = s.amax(1)
        grow = mt if pre else (mt - m) * c
        trig = (grow > thr).view(W, WAVE).any(1)
        if t == 0:
            trig[:] = True
        else:
            fired |= {(t, w) for w in range(W) if trig[w]}
        tr = trig.repeat_interleave(WAVE)
        if pre:
            d = torch.where(tr, mt if t == 0 else mt.clamp_min(0.0), torch.zeros_like(mt))
            m = m + d
            alpha = torch.exp2(-d) if t else torch.ones_like(d)                # first tile: O and l are still zero
            s = s - d[:, None]
            p = torch.exp2(s)
        else:
            m_new = torch.where(tr, torch.maximum(m, mt), m)
            alpha = torch.exp2((m - m_new) * c)
            m = m_new
            p = torch.exp2(s * c - (m * c)[:, None])
        if defect != "no_l":
            l = l * alpha
        if defect != "no_o":
            o = o * alpha[:, None]
        p16 = p.half().float()
        l = l + (p16 if pre else p).sum(1)
        o = o + p16 @ vp[KT * t:KT * (t + 1)]
    return (o / l[:, None]).half()[:Nq], fired


def _ratio(c, thr=ap.THR, defect=None, after=False):
    x = _probe(c)
    out, fired = restate(x["q"], x["k"], x["v"], c["pre"], thr, defect, x["after"] if after else None)
    ratio, _ = lg.bound_ratio(out, x["ref"], x["bound"])
    return float(ratio.max()), out, fired


def _group(*gs, tail=None):
    return [c for c in CASES if c["group"] in gs and (tail is None or (c["Nk"] % KT != 0) == tail)]


def _ids(cs):
    return [c["id"] for c in cs]


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_clean_restatement_stays_inside_half_the_bound(c):
    for thr in ((7.9, 8.1) if c["free"] else (ap.THR,)):
        worst, _, _ = _ratio(c, thr)
        assert worst <= 0.5, (c["id"], thr, worst)


def test_near_threshold_cases_take_both_paths():
    """Growth 8 +- 2^-6 as built (fp64, after the fp16 rounding of the planted key), and the two thresholds of condition A really differ."""
    near = [c for c in CASES if c["free"]]
    assert len(near) == 4
    for c in near:
        x = _probe(c)["x"]
        s = ap.log2_scores(x)
        for p in c["plants"]:
            r, j = p["rows"][0], p["key"]
            grow = s[:, :, r, j] - s[:, :, r, :KT].amax(-1)
            assert ((grow - p["T"][0]).abs() < 2.0 ** -9).all(), (c["id"], p, grow)
        lo, hi = _ratio(c, 7.9)[2], _ratio(c, 8.1)[2]
        assert lo == {(2, w) for w in range(4)} and not hi, (c["id"], lo, hi)


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["mask_long", "mask_short"])
@pytest.mark.parametrize("c", _group("a", tail=True), ids=_ids(_group("a", tail=True)))
def test_tail_mask_off_by_one_key_leaves_the_bound(c, defect):
    worst, _, _ = _ratio(c, defect=defect)
    assert worst > 1.0, (c["id"], defect, worst)


@pytest.mark.parametrize("defect", ["no_o", "no_l"])
@pytest.mark.parametrize("c", _group("c"), ids=_ids(_group("c")))
def test_missing_rescale_leaves_the_bound(c, defect):
    worst, _, fired = _ratio(c, 7.9 if c["free"] else ap.THR, defect)          # a near-threshold case: the path that rescales
    assert fired and worst > 1.0, (c["id"], defect, worst)


_MOVED = [c for c in CASES if c["Nk"] > 4]


@pytest.mark.parametrize("c", _MOVED, ids=_ids(_MOVED))
def test_vt_block_order_left_out_leaves_the_bound(c):
    worst, _, _ = _ratio(c, defect="vt_order")
    assert worst > 1.0, (c["id"], worst)


@pytest.mark.parametrize("c", _group("a", "b", "d", tail=True), ids=_ids(_group("a", "b", "d", tail=True)))
def test_rows_after_the_keys_in_place_of_the_zero_tail(c):
    clean = _ratio(c)[1]
    masked = _ratio(c, after=True)[1]
    assert torch.equal(clean.view(torch.int16), masked.view(torch.int16)), c["id"]     # behind a correct mask nothing can show
    worst, _, _ = _ratio(c, defect="next_tail", after=True)
    assert worst > 1.0, (c["id"], worst)


def test_every_group_is_what_a_defect_test_needs():
    """Removing a group of GPU cases empties the parametrisation of a test above without failing it; this names what is missing."""
    n = {g: len(_group(g)) for g in "abcde"}
    assert n == dict(a=42, b=32, c=52, d=2, e=1), n
    for pre in (0, 1):
        assert {c["Nk"] for c in _group("a") if c["pre"] == pre} == {KT * (nt - 1) + 1 for nt in range(1, 8)} | {KT * nt - 1 for nt in range(1, 8)} | \
            {KT * nt for nt in range(1, 8)}
        assert {(c["B"], c["Nq"]) for c in _group("b") if c["pre"] == pre} == {(B, n) for B in (1, 9) for n in (1, 31, 32, 33, 127, 128, 129, 257)}
        names = {c["id"].split("-", 2)[2] for c in _group("c") if c["pre"] == pre}
        for Nk in (129, 200, 300) if pre else (300,):
            nt = -(-Nk // KT)
            assert {f"N{Nk}_t{t}_T{T}" for t in range(1, nt) for T in (12, 40)} <= names, (pre, Nk)
            assert {f"N{Nk}_consecutive_t{t}" for t in range(1, nt - 1)} | {f"N{Nk}_t{nt - 2}_T200"} <= names, (pre, Nk)
        assert {"N300_t2_own_half", "N300_t2_partner_half", "N300_t3_mate200", "N440_ramp", "N300_t2_near_above", "N300_t2_near_below"} <= names, pre
    assert {(c["B"] * c["H"], c["Nq"], c["Nk"], c["pre"]) for c in _group("d")} == {(576, 40, 40, 1), (576, 40, 129, 1)}


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_predicted_crossings_are_the_restatement_s(c):
    x = _probe(c)
    trig, dist = ap.predict_crossings(x["x"])
    if not c["plants"]:
        assert not trig.any(), c["id"]
    if c["free"]:
        return                                                                  # either path is legal there
    assert (dist[trig] >= 3.9).all() and (dist[~trig] >= 0.5).all(), (c["id"], float(dist[trig].min()) if trig.any() else None, float(dist[~trig].min()))
    b, h = c["probe"]
    want = {(t, w) for t, w in trig[b, h].nonzero().tolist()}
    assert _ratio(c)[2] == want, (c["id"], want)
    if c["group"] == "c":
        assert want, c["id"]


def test_plants_land_where_the_case_says():
    """The rescale cases trigger in the planted tiles, in all four waves of every (image, head), and nowhere else."""
    for c in _group("c"):
        if c["free"]:
            continue
        trig, _ = ap.predict_crossings(_probe(c)["x"])
        tiles = sorted({p["key"] // KT for p in c["plants"]} - {0})
        got = {t for t in range(trig.shape[2]) if trig[:, :, t].any()}
        if "ramp" in c["id"]:
            assert tiles == [1, 2, 3, 4, 5, 6] and got == {2, 4, 6}, (c["id"], got)      # +6 per tile: every second tile crosses
        else:
            assert got == set(tiles), (c["id"], got, tiles)
        assert all(trig[:, :, t].all() for t in got), c["id"]
    for c in _group("d"):
        trig, _ = ap.predict_crossings(_probe(c)["x"])
        hit = sorted({b for b in range(c["B"]) if trig[b].any()})
        assert hit == ([] if c["Nk"] == 40 else [5, 33, 66, 71]), (c["id"], hit)          # one tile: the plant is part of the first maximum


def test_rescale_matrix_triggers_in_every_kind_and_stage_of_body():
    hit = {"pipe": set(), "tile": set()}
    for c in _group("c"):
        if c["free"]:
            continue
        nt = -(-c["Nk"] // KT)
        for t, _w in _ratio(c)[2]:
            hit["pipe" if c["pre"] else "tile"].add(ap.pipe_tiles(nt)[t] if c["pre"] else t == nt - 1)
    assert hit["pipe"] == {(kind, stg) for kind in (0, 1, 2) for stg in (0, 1)}, hit
    assert hit["tile"] == {False, True}, hit                                    # the one-tile kernel: a middle tile and the masked last tile
    assert [ap.pipe_tiles(n) for n in (1, 2, 3, 4)] == [[(2, 0)], [(1, 0), (2, 1)], [(0, 0), (1, 1), (2, 0)], [(0, 0), (0, 1), (1, 0), (2, 1)]]
