"""The guarded-layout GPU matrix (tests/test_kernel_layouts_gpu.py) stays complete: every GEMM, linear_f32, LayerNorm and attention
descriptor that the V2 (vits14, vitl14) and V1 (cnvnxtl) launch programs record on the host falls into a class the GPU module covers, so
a product path cannot appear without a guarded GPU test.  Nothing runs on a device: the plans are recorded with host tensors standing in
for the device buffers (the dry runs of tests/test_host_cpu.py)."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("test_kernel_layouts_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_kernel_layouts_gpu.py"))
lay = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lay)
_spec = importlib.util.spec_from_file_location("dry_run", os.path.join(os.path.dirname(os.path.abspath(__file__)), "dry_run.py"))
dry_run = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dry_run)

PLANS = (("v2", "vits14"), ("v2", "vitl14"), ("v1", "cnvnxtl"))


def _record(kind, arch):
    seen = {k: [] for k in ("gemm", "linear_f32", "layernorm", "attention")}

    def log(name):
        def add(real, h, dref):
            seen[name].append(type(dref._obj).from_buffer_copy(dref._obj))
            return real(h, dref)
        return add
    with dry_run.host_recording({name: log(name) for name in seen}):
        if kind == "v2":
            dry_run.v2_model(arch, 3, 2)._plan(1, 462, 616, 0, True, True)
        else:
            dry_run.v1_model(arch, 301)._full_plan(1, 240, 320, True, False, True, 0, False)
    return seen


@pytest.fixture(scope="module")
def recorded():
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    return {f"{k}/{a}": _record(k, a) for k, a in PLANS}


def test_gemm_cases_reach_the_schedule_they_name():
    """Each GPU case's descriptor, built on the host, picks the schedule the case declares -- at every layout it runs."""
    from unidepth_amd import _lib
    bad = [(c["id"], lo, _lib.lib.ud_gemm_pick(C.byref(lay.host_desc(c, lo)))) for c in lay.GEMM_CASES for lo in lay._lay(c)
           if _lib.lib.ud_gemm_pick(C.byref(lay.host_desc(c, lo))) != c["pick"]]
    assert not bad, bad
    picks = {c["pick"] for c in lay.GEMM_CASES}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 19, 20, 36} <= picks
    hints = {c.get("hint", 0) for c in lay.GEMM_CASES}
    assert {1, 2, 3, 5, 7, 8, 9, 10, 11, 12, 13, 14} <= hints           # every tile_hint of include/unidepth_hip.h (6: the auto ring cases)


def test_every_product_gemm_class_has_a_guarded_gpu_case(recorded):
    declared = lay.declared_gemm_classes()
    for plan, seen in recorded.items():
        assert len(seen["gemm"]) > 60, plan
        missing = sorted({lay.gemm_class(d) for d in seen["gemm"]} - declared)
        assert not missing, (plan, missing)


@pytest.mark.parametrize("op,flags,table", [("linear_f32", "linear_flags", "LINEAR_F32_FLAGS"), ("layernorm", "layernorm_flags", "LAYERNORM_FLAGS"),
                                            ("attention", "attention_flags", "ATTENTION_FLAGS")])
def test_every_product_descriptor_stride_class_is_covered(recorded, op, flags, table):
    f, declared = getattr(lay, flags), getattr(lay, table)
    n = 0
    for plan, seen in recorded.items():
        n += len(seen[op])
        missing = sorted({f(d) for d in seen[op]} - declared)
        assert not missing, (plan, op, missing)
    assert n > 0, op
