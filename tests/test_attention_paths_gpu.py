"""ud_attention_f16 as a function of TILE COUNT and of SCORE VALUES, element by element (tests/layout_guard.py).

tests/test_kernel_layouts_gpu.py runs the attention kernels at every stride class on randn operands.  What those inputs cannot see is
what this module builds inputs for:

  the key-tail mask   the K descriptor ends after key Nk - 1, so the keys of the last tile past Nk arrive as ZEROS and only the mask keeps
                      them out of the softmax.  On randn rows a zero score is one key among Nk; here a third of the query rows have every
                      real score near -12 (log2 units), so one zero "phantom" key outweighs all of them;
  the tile count      every branch of the pipelined kernel's tile loop (nt = 1 .. 7, with and without a tail), a single-tile item with a
                      successor, fewer (image, head) pairs than XCDs;
  the rescale path    a planted key lifts ONE row's score by a stated amount above its running maximum in a stated tile, so the deferred
                      maximum (threshold 2^8) triggers in a known (tile, wave) -- in every KIND x stage of the pipelined body().

Inputs (make_inputs): head dim 64, dimension 0 is reserved -- K[:, 0] = 1 and Q[i, 0] = sigma_i in log2 units, sigma cycling over
{-12, 0, +12} by query row -- and dimensions 1..63 are randn scaled so that the rest of the score has a standard deviation of ~1.4 log2
units.  Raw Q (the one-tile kernel) is the same divided by scale log2(e), rounded to fp16 BEFORE anything else is derived from it.  A plant
sets the score of (row i, key j) to a target by K[j] = q_i T / |q_i|^2 from the rounded q (the Gram system when one key serves several
rows: the last tile of Nk = 129 has one key), and predict_crossings() states from the fp64 scores which (tile, wave) pairs cross.  V is
randn with |element| >= 2^-4: the bound has no term for the absolute error of an fp16-subnormal P, and make_inputs says why that floor
makes it none the looser.

The bound (attention_bound) is a sum of named terms, none of them tuned on a kernel's output:
    2^-11 |ref| + 2^-25                           the fp16 store
  + (2^-10                                        fp16 rounding of P, numerator and denominator
     + ln2 ds_i                                   the fp32 score: ds_i = 2 C_ACC sqrt(64) 2^-24 max_j sum_d |q_id| |k_jd| in log2 units (the
                                                  factor 2: the offset subtraction or, for raw Q, the fma(s, c, -m c))
     + C_ACC sqrt(Nk) 2^-24) mag                  the fp32 accumulation over the keys;  mag = P |V|
tests/test_attention_bounds_cpu.py holds the conditions this module's inputs and bound must meet with no GPU: a torch restatement of both
kernels stays inside half of it, every planted defect leaves it, and the predicted crossings are the restatement's.

Every case prints `RATIO attention <case> <worst error / bound>`.  The module imports without a GPU."""
import importlib.util
import math
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("layout_guard", os.path.join(os.path.dirname(os.path.abspath(__file__)), "layout_guard.py"))
lg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lg)

pytestmark = pytest.mark.gpu

KT = 64                         # keys per tile
WAVE = 32                       # query rows per wave
THR = 8.0                       # the deferred-maximum threshold, log2 units
SCALE = 0.125
LOG2E = 1.4426950408889634
SIGMA = (-12.0, 0.0, 12.0)      # Q[i, 0] by i % 3, log2 units
AMP = 0.42                      # dimensions 1..63 of q and k: 63 AMP^4 = 1.4^2
V_FLOOR = 2.0 ** -4             # smallest |V| element (see make_inputs)
Q_PAD, K_PAD = 3, 5             # rows per image past Nq / Nk (q_rows_per_img, k_rows_per_img > N)


def pipe_tiles(nt):
    """(KIND, stage) of body() for every tile of attention_pipe_kernel: KIND 0 steady, 1 tile nt-2, 2 tile nt-1."""
    out, t = [], 0
    while t + 4 <= nt:
        out += [(0, 0), (0, 1)]
        t += 2
    return out + {3: [(0, 0), (1, 1), (2, 0)], 2: [(1, 0), (2, 1)], 1: [(2, 0)]}[nt - t]


def _row(w, cls, off=0):
    """The first query row >= 32 w + off with sigma class `cls` (0: -12, 1: 0, 2: +12)."""
    r = WAVE * w + off
    return r + (cls - r) % 3


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
# keys: id group B H Nq Nk pre (q_prescaled: 1 the pipelined kernel, 0 the one-tile kernel on raw Q) seed
#       plants: dict(key, rows, T, base, imgs, lowest) in planting order -- the score of (row, key) becomes base + T, base = the row's tile-0
#               maximum at planting time ("tile0") or the row's previous planted score ("prev"); imgs None = every image
#       probe: the (image, head) tests/test_attention_bounds_cpu.py restates;  free: either path is legal (the near-threshold cases)
CASES = []
_SPREAD = (3, 21, 34, 60)       # in-tile key index per wave: key % 8 = 3, 5, 2, 4 (both lane halves)
_OFFS = (5, 12, 20, 27)         # row offset inside the wave, per wave


def _add(group, name, B, H, Nq, Nk, pre, plants=(), probe=None, free=False):
    CASES.append(dict(id=f"{group}-{'pipe' if pre else 'tile'}-{name}", group=group, B=B, H=H, Nq=Nq, Nk=Nk, pre=pre, plants=list(plants),
                      probe=probe or (B - 1, H - 1), free=free, seed=1000 + len(CASES)))


def _tile_plants(Nk, t, T, cls=1, idx=_SPREAD, base="tile0", waves=4, lowest=False):
    """One plant per wave in tile t: row _row(w, cls, _OFFS[w]), key 64 t + idx[w] (folded into the tile's valid keys; one shared key -- the
    Gram form -- where the tile has too few)."""
    nv = min(KT, Nk - KT * t)
    assert nv >= 1
    keys = [KT * t + i % nv for i in idx[:waves]]
    rows = [_row(w, cls, _OFFS[w]) for w in range(waves)]
    if len(set(keys)) < len(keys):
        return [dict(key=keys[0], rows=rows, T=[T] * len(rows), base=base)]
    return [dict(key=k, rows=[r], T=[T], base=base, lowest=lowest) for k, r in zip(keys, rows)]


for _pre in (1, 0):
    # a. tile-count matrix: two pairs (six XCDs idle), wave 1 holds one row, waves 2-3 are clamped
    for _nt in range(1, 8):
        for _Nk in (KT * (_nt - 1) + 1, KT * _nt - 1, KT * _nt):
            _add("a", f"nt{_nt}_Nk{_Nk}", 1, 2, 33, _Nk, _pre)
    # b. query edges
    for _B in (1, 9):
        for _Nq in (1, 31, 32, 33, 127, 128, 129, 257):
            _add("b", f"B{_B}_Nq{_Nq}", _B, 1, _Nq, 65, _pre)
    # c. rescale matrix: in every wave one sigma = 0 row is lifted T above its tile-0 maximum by a key of tile t
    for _Nk in ((129, 200, 300) if _pre else (300,)):
        _ntc = -(-_Nk // KT)
        for _t in range(1, _ntc):
            for _T in (12, 40):
                _add("c", f"N{_Nk}_t{_t}_T{_T}", 2, 4, 128, _Nk, _pre, _tile_plants(_Nk, _t, _T))
        _add("c", f"N{_Nk}_t{_ntc - 2}_T200", 2, 4, 128, _Nk, _pre, _tile_plants(_Nk, _ntc - 2, 200))
        # tiles t and t + 1 of the same row, the second 12 above the first
        for _t in range(1, _ntc - 1):
            _add("c", f"N{_Nk}_consecutive_t{_t}", 2, 4, 128, _Nk, _pre, _tile_plants(_Nk, _t, 12) + _tile_plants(_Nk, _t + 1, 12, base="prev"))
    # the lane's own keys (key % 8 < 4) / the partner lane's (key % 8 >= 4)
    _add("c", "N300_t2_own_half", 2, 4, 128, 300, _pre, _tile_plants(300, 2, 40, idx=(1, 10, 19, 56)))
    _add("c", "N300_t2_partner_half", 2, 4, 128, 300, _pre, _tile_plants(300, 2, 40, idx=(4, 13, 22, 63)))
    # a wave-mate whose maximum is a +200 key of tile 0 (its later mt is ~ -200 while another row triggers): d = max(mt, 0)
    for _Nk, _t in ((300, 3), (129, 1)) if _pre else ((300, 3),):
        _add("c", f"N{_Nk}_t{_t}_mate200", 2, 4, 128, _Nk, _pre,
             [dict(key=40 + w, rows=[_row(w, 1, 1)], T=[200], base="tile0") for w in range(4)] + _tile_plants(_Nk, _t, 40))
    # a ramp: a sigma = +12 row's maximum grows by 6 per tile over seven tiles (a trigger every second tile)
    _add("c", "N440_ramp", 2, 4, 128, 440, _pre, [p for t in range(1, 7) for p in _tile_plants(440, t, 6 * t, cls=2)])
    # growth 8 +- 2^-6: either path is legal, only the bound is asserted
    _add("c", "N300_t2_near_above", 2, 4, 128, 300, _pre, _tile_plants(300, 2, THR + 2.0 ** -6, cls=2, lowest=True), free=True)
    _add("c", "N300_t2_near_below", 2, 4, 128, 300, _pre, _tile_plants(300, 2, THR - 2.0 ** -6, cls=2, lowest=True), free=True)
# d. persistent walk: 576 pairs = 72 items per XCD against 64 slots; planted rows in images whose items are a workgroup's first (pair < 512)
#    and its second (image >= 64), in tile 0 and in the last tile
for _Nk in (40, 129):
    _add("d", f"Nk{_Nk}", 72, 8, 40, _Nk, 1,
         [dict(key=7, rows=[_row(0, 1, 4)], T=[40], base="tile0", imgs=[2, 40, 64, 67]),
          dict(key=_Nk - 2 if _Nk == 40 else _Nk - 1, rows=[_row(0, 1, 9), _row(1, 1, 4)], T=[40, 40], base="tile0", imgs=[5, 33, 66, 71])],
         probe=(66, 3))
# e. a schedule class a recorded product plan reaches (tests/test_layout_coverage_cpu.py) and no case above: the steady loop, three tiles
#    after it, no key tail, at least one pair per XCD, two q-tiles per pair
_add("e", "nt7_Nk448_pairs8", 2, 4, 130, 448, 1)
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _ulp16(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14))) - 10)


def make_inputs(c):
    """Host tensors of case `c`: q [B, H, Nq, 64] fp16 AS THE KERNEL GETS IT (log2 units when pre-scaled, raw otherwise), k, v [B, H, Nk, 64]
    fp16, k_pad [B, H, K_PAD, 64] (the rows after an image's keys: loud finite keys no kernel may read into a result) and `cq`, the factor
    that turns q k into log2 units.

    V is randn with every |element| raised to at least V_FLOOR = 2^-4 (the sign kept).  Both kernels hold P in fp16, and a P below 2^-14
    of the row's offset is an fp16 SUBNORMAL: its rounding error is absolute, up to 2^-25 per key, and the bound has no term for it --
    every P term there is relative to mag = P |V|.  The row sum is >= 1, so over a row these errors add up to at most Nk 2^-25 max|V|
    (448 keys, |V| < 4.5: 6e-5, typically sqrt(Nk) 2^-25 ~ 6e-7), which is nothing next to 2^-10 mag unless one key holds the whole row AND
    its V element is itself near zero: a planted key over a 2e-5 element of randn V gave 2.5 x the bound in the torch restatement, the
    kernel returning that key's V element to the bit.  With |V| >= 2^-4, mag >= 2^-4 and 2^-10 mag >= 2^-14 = 6.1e-5 covers even the
    worst-case sum, so the bound as derived holds for a correct kernel on every input built here."""
    B, H, Nq, Nk, pre = c["B"], c["H"], c["Nq"], c["Nk"], c["pre"]
    g = torch.Generator().manual_seed(c["seed"])
    cq = 1.0 if pre else SCALE * LOG2E
    q = torch.randn(B, H, Nq, 64, generator=g, dtype=torch.float64) * AMP
    q[..., 0] = torch.tensor(SIGMA, dtype=torch.float64)[torch.arange(Nq) % 3]
    q = (q / cq).half()                                                        # rounded before anything is derived from it
    qe = q.double() * cq
    kd = torch.randn(B, H, Nk, 64, generator=g, dtype=torch.float64) * AMP
    kd[..., 0] = 1.0
    kd = kd.half().double()
    v = torch.randn(B, H, Nk, 64, generator=g, dtype=torch.float64)
    v = torch.where(v.abs() < V_FLOOR, torch.full_like(v, V_FLOOR).copysign(v), v).half()
    k_pad = torch.randn(B, H, K_PAD, 64, generator=g, dtype=torch.float64) * 2.0
    k_pad[..., 0] = -4.0                                                       # loud for the sigma = -12 rows, which every case has
    last = {}
    for p in c["plants"]:
        imgs = torch.arange(B) if p.get("imgs") is None else torch.tensor(p["imgs"])
        rows, j = p["rows"], p["key"]
        assert 0 <= j < Nk and all(0 <= r < Nq for r in rows), (c["id"], p)
        if p.get("lowest"):
            assert len(rows) == 1 and p.get("imgs") is None
            # the planted row becomes the one of its wave and sigma class with the SMALLEST tile-0 maximum (two iid rows swap places): the key
            # gives every sigma = +12 row 0.93 of the planted score, which then stays below the planted row's own growth by > 1
            r0 = rows[0]
            cand = torch.tensor([r for r in range(WAVE * (r0 // WAVE), min(Nq, WAVE * (r0 // WAVE + 1))) if r % 3 == r0 % 3])
            lowest = cand[(qe[:, :, cand] @ kd[:, :, :min(KT, Nk)].transpose(-1, -2)).amax(-1).argmin(-1)]
            idx = lowest[..., None, None].expand(-1, -1, 1, 64)
            for ten in (q, qe):
                mine, other = ten[:, :, r0].clone(), ten.gather(2, idx).squeeze(2)
                ten.scatter_(2, idx, mine.unsqueeze(2))
                ten[:, :, r0] = other
        Qs = qe[imgs][:, :, rows]                                              # [n, H, R, 64]
        if p["base"] == "tile0":
            base = (Qs @ kd[imgs][:, :, :min(KT, Nk)].transpose(-1, -2)).amax(-1)
        else:
            base = torch.stack([last[r] for r in rows], -1)
        target = base + torch.tensor(p["T"], dtype=torch.float64)
        a = torch.linalg.solve(Qs @ Qs.transpose(-1, -2), target.unsqueeze(-1))   # one row: a = T / |q|^2
        kj = (a.transpose(-1, -2) @ Qs).squeeze(-2).half().double()            # [n, H, 64]
        if len(rows) == 1:                                                     # ulp steps of single elements: the fp16 key meets the target to ~2^-9
            qi = Qs[:, :, 0]
            mult = torch.cat([2.0 ** torch.arange(9), -(2.0 ** torch.arange(9))]).double()
            for _ in range(24):
                err = (target[..., 0] - (qi * kj).sum(-1))[..., None, None]      # [n, H, 1, 1]
                ulp = _ulp16(kj)
                cand = (qi * ulp).unsqueeze(-1) * mult                           # +- 1 .. 256 ulps of every element
                best = (err - cand).abs().flatten(-2).argmin(-1, keepdim=True)
                d, n = best // mult.numel(), mult[best % mult.numel()]
                gain = (err.squeeze(-1) - cand.flatten(-2).gather(-1, best)).abs() < err.squeeze(-1).abs()
                kj.scatter_add_(-1, d, torch.where(gain, n * ulp.gather(-1, d), torch.zeros_like(n)))
                kj = kj.half().double()
        kd[imgs, :, j] = kj
        got = (Qs @ kj.unsqueeze(-1)).squeeze(-1)
        for n, r in enumerate(rows):
            last[r] = got[..., n]
    return dict(q=q, k=kd.half(), v=v, k_pad=k_pad.half(), cq=cq)


def log2_scores(x):
    return (x["q"].double() * x["cq"]) @ x["k"].double().transpose(-1, -2)


def predict_crossings(x, thr=THR):
    """From the fp64 scores: trig [B, H, nt, waves] -- the deferred maximum of that wave triggers in that tile (tile 0 always does and is
    left False) -- and dist, |the wave's largest growth - thr| (inf for tile 0).  A wave triggers when ANY of its rows grew by more than
    thr; every row of a triggering wave then moves its offset by max(growth, 0)."""
    s = log2_scores(x)
    B, H, Nq, Nk = s.shape
    nt, W = -(-Nk // KT), -(-Nq // WAVE)
    wave = torch.arange(Nq) // WAVE
    m = s[..., :KT].amax(-1)
    trig = torch.zeros(B, H, nt, W, dtype=torch.bool)
    dist = torch.full((B, H, nt, W), math.inf, dtype=torch.float64)
    for t in range(1, nt):
        mt = s[..., KT * t:KT * (t + 1)].amax(-1) - m
        for w in range(W):
            wmax = mt[..., wave == w].amax(-1)
            trig[:, :, t, w] = wmax > thr
            dist[:, :, t, w] = (wmax - thr).abs()
        m = m + torch.where(trig[:, :, t][..., wave], mt.clamp_min(0.0), torch.zeros_like(mt))
    return trig, dist


# ---- reference and bound ------------------------------------------------------------------------------------------------------------------
def attention_bound(q, k, v, cq):
    """fp64 reference of softmax(q k^T) v on the rounded operands [..., N, 64] (q k in log2 units after the factor cq) and the bound of the
    module docstring; returns (ref, bound, terms by name)."""
    q, k, v = q.double() * cq, k.double(), v.double()
    Nk = k.shape[-2]
    p = torch.softmax(q @ k.transpose(-1, -2) * math.log(2.0), -1)
    ref, mag = p @ v, p @ v.abs()
    ds = 2.0 * lg.C_ACC * math.sqrt(64.0) * 2.0 ** -24 * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    terms = dict(store=lg.term_store_f16(ref), p_f16=2.0 ** -10 * mag, score=math.log(2.0) * ds * mag, accumulate=lg.term_rounding(mag, Nk))
    return ref, sum(terms.values()), terms


# ---- GPU side -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unidepth_amd import ops as _ops
    return _ops


def run_case(ops, c):
    """Run case `c`; every output element against the bound, every guard element bitwise.  Returns the worst error / bound."""
    B, H, Nq, Nk, pre = c["B"], c["H"], c["Nq"], c["Nk"], c["pre"]
    x = {n: (t.cuda() if torch.is_tensor(t) else t) for n, t in make_inputs(c).items()}
    D, qr, kr = H * 64, Nq + Q_PAD, Nk + K_PAD
    kv64 = (Nk + KT - 1) // KT * KT
    kv_ld = kv64 + 64
    Q = torch.full((B, qr, H, 64), float("nan"), dtype=torch.half, device="cuda")              # rows past Nq: poison
    Q[:, :Nq] = x["q"].permute(0, 2, 1, 3)
    K = torch.empty(B, kr, H, 64, dtype=torch.half, device="cuda")
    K[:, :Nk] = x["k"].permute(0, 2, 1, 3)
    K[:, Nk:] = x["k_pad"].permute(0, 2, 1, 3)                                                 # rows past Nk: loud finite keys
    Kb = lg.poisoned(K.view(B * kr, D), post_rows=KT, fill=-4.0)                                # ... and after the last image
    vt = torch.zeros(B, H, 64, kv_ld, dtype=torch.half, device="cuda")                         # [Nk, kv64): the zeros the header requires
    vt[..., kv64:] = float("nan")
    vt[..., lg.vt_cols(Nk).cuda()] = x["v"].transpose(-1, -2)
    ldo = D + 64
    go = lg.guarded(B * qr, D, ldo, torch.half, offset_cols=8, rows_inside=torch.cat([b * qr + torch.arange(Nq) for b in range(B)]).cuda())
    ops.attention(Q=Q, K=Kb, Vt=vt, O=go.view, B=B, H=H, Nq=Nq, Nk=Nk, ldq=D, ldk=D, ldo=ldo, kv_ld=kv_ld, q_rows_per_img=qr,
                  k_rows_per_img=kr, scale=SCALE, kv_broadcast=0, kv_group=0, q_prescaled=pre)
    torch.cuda.synchronize()
    ref, bound, _ = attention_bound(x["q"], x["k"], x["v"], x["cq"])
    out = go.view.reshape(B, qr, H, 64)[:, :Nq].permute(0, 2, 1, 3)
    worst = lg.assert_bound(out, ref, bound, name=f"{c['id']} O[image, head, row, d]")
    go.check_guards("O")
    print(f"RATIO attention {c['id']} {worst:.4f}")
    return worst


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_attention_paths(ops, c):
    """Groups a (tile count x key tail), b (query edges), c (the rescale path in a stated tile and wave), d (the persistent walk) and e (a
    product plan's schedule class), both kernels: every element of every (image, head) inside the bound, the pad rows of O and its stride gaps intact."""
    run_case(ops, c)
