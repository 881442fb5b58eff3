"""Host-only coverage check of tests/knn_cases.py: every kernel class ud_knn_points can dispatch to (csrc/evalops.hip) keeps at least one
case, and every case reaches the split / unsplit path it declares.  Nothing is launched: ud_knn_split is a host function.  Every
case of the table is the only one of its class, so deleting any one fails test_every_knn_kernel_class_keeps_a_case or
test_every_tie_and_overflow_class_keeps_a_case with the class's name."""
import numpy as np
import pytest

import knn_cases as kc


@pytest.fixture(scope="module")
def classes():
    return {c["id"]: kc.knn_class(c) for c in kc.CASES}


def test_every_knn_kernel_class_keeps_a_case(classes):
    """by the plain random cases alone: the tie and overflow cases below do not stand in for them"""
    plain = [(c, classes[c["id"]]) for c in kc.CASES if c["data"] == "randn"]
    knn = {(dc, kt, split) for _, (fam, dc, kt, _, split) in plain if fam == "knn"}
    fast1 = {(norm, split) for c, (fam, _, _, norm, split) in plain if fam == "fast1" and c["D"] == 3}
    assert len(kc.REQUIRED_KNN) == 26 and len(kc.REQUIRED_FAST1) == 4
    missing = sorted(f"knn_kernel<{dc},{kt}>{' split' if s else ''}" for dc, kt, s in kc.REQUIRED_KNN - knn)
    missing += sorted(f"knn1_d3_kernel<{'true' if n == 2 else 'false'}>{' split' if s else ''}" for n, s in kc.REQUIRED_FAST1 - fast1)
    assert not missing, missing
    assert any(fam == "fast1" and split and c["D"] < 3 for c, (fam, _, _, _, split) in plain), "fast1 split with D < 3 (tile staging)"
    for dc in (3, 4, 8, 0):                # per DC: both norms, K equal to KT and K strictly inside KT's bracket
        mine = [(c, cl) for c, cl in plain if cl[0] == "knn" and cl[1] == dc]
        assert {cl[3] for _, cl in mine} == {1, 2}, dc
        assert any(c["K"] == cl[2] for c, cl in mine) and any(cl[2] // 2 < c["K"] < cl[2] for c, cl in mine), dc
    assert {c["D"] for c, cl in plain if cl[0] == "knn" and cl[1] == 3} == {1, 2, 3}
    assert {c["D"] for c, cl in plain if cl[0] == "knn" and cl[1] == 8} == {5, 8}
    assert {c["D"] for c, cl in plain if cl[0] == "knn" and cl[1] == 0} == {9, 32}


def test_every_tie_and_overflow_class_keeps_a_case(classes):
    """ties: three patterns x (fast1, both norms, split and unsplit) and K = 4 on DC = 4; +inf distances: K = 1 on D = 3 and D = 4, split
    and unsplit, and K = 4"""
    have = set()
    for c in kc.CASES:
        fam, dc, kt, norm, split = classes[c["id"]]
        if c["data"] != "randn":           # the norm counts on fast1, where it is a template argument
            have.add((c["data"], fam, dc, kt, norm, split) if fam == "fast1" else (c["data"], fam, dc, kt, split))
    want = {(data, "fast1", 3, 1, norm, split) for data in ("twin_half", "twin_next", "lattice") for norm in (1, 2) for split in (False, True)}
    want |= {(data, "knn", 4, 4, False) for data in ("twin_half", "twin_next", "lattice")}
    want |= {("overflow", "fast1", 3, 1, 2, split) for split in (False, True)} | {("overflow", "knn", 4, 1, split) for split in (False, True)}
    want |= {("overflow", "knn", 3, 4, False), ("overflow", "knn", 4, 4, False)}
    assert not want - have, sorted(want - have)
    assert len(kc.CASES) == 24 + 5 + 3 + 15 + 6


@pytest.mark.parametrize("case", kc.CASES, ids=[c["id"] for c in kc.CASES])
def test_case_reaches_the_path_it_declares(case, classes):
    S = kc.knn_split(case)
    assert (S > 1) == case["split"], S
    assert classes[case["id"]][4] == case["split"]
    if case["split"]:                      # the span of a slice is not a multiple of the 1024-point tile (nor of the 8-point chunk)
        span = -(-case["P2"] // S)
        assert S == 3 and span % 8 != 0, (S, span)
    if case["id"] in kc.GUARDED:
        assert case["data"] == "randn"


def test_guarded_cases_cover_every_family(classes):
    fams = {(classes[i][0], classes[i][1] if classes[i][0] == "knn" else 3, classes[i][4]) for i in kc.GUARDED}
    assert fams >= {("fast1", 3, False), ("fast1", 3, True), ("knn", 3, False), ("knn", 4, False), ("knn", 8, False), ("knn", 0, False)}
    assert any(f[0] == "knn" and f[2] for f in fams)


@pytest.mark.parametrize("case", kc.CASES, ids=[c["id"] for c in kc.CASES])
def test_lengths_follow_the_rule(case):
    P1, P2, K = case["P1"], case["P2"], case["K"]
    per = kc.queries_per_block(case)
    short = K - 1 if K > 1 else 5
    searched = []
    for variant in kc.VARIANTS:
        l1, l2 = (v.tolist() for v in kc.lengths(case, variant))
        mid = sorted(l1)[1]
        assert sorted(l1) == [0, mid, P1] and (P1 - 1) // per * per < mid < P1      # strictly inside the last query block
        assert sorted(l2) == [0, short, P2]
        assert all(a or b for a, b in zip(l1, l2))                                  # no cloud empty on both sides
        searched += [(a, b) for a, b in zip(l1, l2) if a and b]
    assert sorted(searched) in ([(mid, short), (P1, P2)], [(mid, P2), (P1, short)])  # one full and one short search per case


def test_tie_and_overflow_inputs_are_what_they_claim():
    for case in kc.CASES:
        p1, p2 = kc.inputs(case)
        P2 = case["P2"]
        if case["data"] == "twin_half":
            assert np.array_equal(p2[:, :P2 // 2].numpy(), p2[:, P2 // 2:].numpy())
        elif case["data"] == "twin_next":
            assert np.array_equal(p2[:, 0:512:2].numpy(), p2[:, 1:512:2].numpy())
            assert np.array_equal(p2[:, 513:P2 - 1:2].numpy(), p2[:, 514:P2:2].numpy())     # (1023, 1024) among them
        elif case["data"] == "lattice":
            assert set(np.unique(p2.numpy())) <= {0.0, 1.0, 2.0, 3.0}
        elif case["data"] == "overflow":
            d, _ = kc.reference(case)
            l1, l2 = kc.lengths(case)
            for n in range(kc.N):
                if l1[n] and l2[n]:
                    kv = min(case["K"], int(l2[n]))
                    assert np.isposinf(d[n, list(kc.OVERFLOW_ROWS), :kv]).all() and np.isfinite(d[n, 2:int(l1[n])]).all()
