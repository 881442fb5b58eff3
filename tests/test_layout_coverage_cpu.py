"""The guarded-layout GPU matrix (tests/test_kernel_layouts_gpu.py) stays complete: every GEMM, linear_f32, LayerNorm and attention
descriptor that the V2 (vits14, vitl14) and V1 (cnvnxtl) launch programs record on the host falls into a class the GPU module covers, so
a product path cannot appear without a guarded GPU test.  Nothing runs on a device: the plans are recorded with host tensors standing in
for the device buffers (the dry runs of tests/test_host_cpu.py)."""
import contextlib
import ctypes as C
import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("test_kernel_layouts_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_kernel_layouts_gpu.py"))
lay = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lay)

PLANS = (("v2", "vits14"), ("v2", "vitl14"), ("v1", "cnvnxtl"))


def _record(monkeypatch, kind, arch):
    from unidepth_amd import _lib, ops
    seen = {k: [] for k in ("gemm", "linear_f32", "layernorm", "attention")}
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr()))
    for name in seen:
        real = getattr(_lib.lib, "ud_program_add_" + name)

        def add(h, dref, real=real, name=name):
            seen[name].append(type(dref._obj).from_buffer_copy(dref._obj))
            return real(h, dref)
        monkeypatch.setattr(ops.lib, "ud_program_add_" + name, add)
    dev = torch.device("cpu")
    if kind == "v2":
        from oracle import synth
        from unidepth_amd import UniDepthV2
        from unidepth_amd.weights import pack
        cfg = synth.load_config(arch)
        m = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, 3))
        m._w, m._device, m.resolution_level = pack(cfg, m._sd, dev), dev, 2
        m._plan(1, 462, 616, 0, True, True)
    else:
        from oracle import synth_v1
        from unidepth_amd import UniDepthV1, unidepthv1 as U
        cfg = synth_v1.load_config_v1(arch)
        m = UniDepthV1(cfg).load_state_dict(synth_v1.make_synthetic_checkpoint_v1(cfg, 301))
        m._w, m._device = {**U.pack_convnext(cfg, m._sd, dev), **U.pack_v1_decoder(cfg, m._sd, dev)}, dev
        m._full_plan(1, 240, 320, True, False, True, 0, False)
    monkeypatch.undo()
    return seen


@pytest.fixture(scope="module")
def recorded():
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    mp = pytest.MonkeyPatch()
    try:
        return {f"{k}/{a}": _record(mp, k, a) for k, a in PLANS}
    finally:
        mp.undo()


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
