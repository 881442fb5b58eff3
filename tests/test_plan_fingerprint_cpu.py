"""The launch programs the plan builders record are pinned: tests/golden/plan_fingerprints.json holds, per signature, the fingerprint of
the whole `ud_program_add_*` stream (tools/plan_fingerprint.py: every descriptor field by value, every pointer by allocation and offset,
prog.meta, tap points, shape-policy attributes).  A change of a builder that is meant to leave the programs alone must pass with the
golden file untouched; a change that edits a launch program regenerates it (`python tools/plan_fingerprint.py --write`) and shows the
per-op diff.  Recording also asserts buffer lifetime: every non-weight pointer of the stream falls inside a tensor the plan keeps alive
(`prog.keep` or an attribute).  Nothing runs on a device."""
import importlib.util
import json
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("plan_fingerprint", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                                                                                "plan_fingerprint.py"))
fp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fp)


@pytest.fixture(scope="module")
def models():
    built = {}

    def get(key):                        # one synthetic model per test module and backbone (packing ViT-L on the host takes seconds)
        if key not in built:
            built[key] = fp.MODELS[key]()
        return built[key]
    return get


@pytest.fixture(scope="module")
def golden():
    with open(fp.GOLDEN) as f:
        return json.load(f)


def test_golden_file_pins_exactly_the_listed_signatures(golden):
    assert sorted(golden) == sorted(name for name, _ in fp.SIGNATURES)
    assert all(len(g["lines"]) == g["ops"] > 100 for g in golden.values())


@pytest.mark.parametrize("name,build", fp.SIGNATURES, ids=[name for name, _ in fp.SIGNATURES])
def test_recorded_launch_program_matches_its_fingerprint(models, golden, name, build):
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    got = fp.fingerprint(models(name.split("/")[0]), name, build)      # asserts buffer lifetime while it names the pointers
    assert fp.first_difference(got, golden[name]) is None, fp.first_difference(got, golden[name])
    assert got["sha256"] == golden[name]["sha256"]
