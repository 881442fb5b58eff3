"""The guarded-layout GPU matrices (tests/test_kernel_layouts_gpu.py, tests/test_pointwise_layouts_gpu.py) stay complete: every descriptor
that the V2 (vits14, vitl14) and V1 (cnvnxtl, vitl14) launch programs record on the host -- through ANY ud_program_add_* entry point --
falls into a class one of the two GPU modules covers, so a product path cannot appear without a guarded GPU test.  Nothing runs on a
device: the plans are recorded with host tensors standing in for the device buffers (the dry runs of tests/test_host_cpu.py)."""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch

_spec = importlib.util.spec_from_file_location("test_kernel_layouts_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_kernel_layouts_gpu.py"))
lay = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lay)
_spec = importlib.util.spec_from_file_location("test_pointwise_layouts_gpu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_pointwise_layouts_gpu.py"))
pw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pw)
_spec = importlib.util.spec_from_file_location("dry_run", os.path.join(os.path.dirname(os.path.abspath(__file__)), "dry_run.py"))
dry_run = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dry_run)

PLANS = (("v2", "vits14"), ("v2", "vitl14"), ("v1", "cnvnxtl"), ("v1", "vitl14"))
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "unidepth_hip.h")
ENTRY_POINTS = sorted(set(re.findall(r"ud_program_add_(\w+)\(", open(_HEADER).read())))      # every recording entry point of the C-ABI


def _record(kind, arch):
    seen = {k: [] for k in ENTRY_POINTS}

    def log(name):
        def add(real, h, *a):
            # a descriptor struct is copied (the caller's goes out of scope); scalar argument lists are kept as they are
            seen[name].append(type(a[0]._obj).from_buffer_copy(a[0]._obj) if len(a) == 1 and hasattr(a[0], "_obj") else a)
            return real(h, *a)
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


def test_every_entry_point_is_intercepted(recorded):
    assert len(ENTRY_POINTS) == 23 and {"gemm", "v1_op", "fill_rows", "dwconv7", "finalize"} <= set(ENTRY_POINTS)
    used = {name for seen in recorded.values() for name, calls in seen.items() if calls}
    assert {"fill_rows", "camera_intrinsics", "rays", "ray_embed", "upsample2x", "resize_ac", "nhwc_to_nchw", "dwconv7", "layernorm_patchify2", "patchify4",
            "spatial_mean", "attention_small_f32", "v1_op"} <= used, used


def test_every_product_pointwise_class_has_a_guarded_gpu_case(recorded):
    """Every recorded descriptor outside the GEMM / LayerNorm / attention family maps to a class (op or V1 kind, the flags that pick a kernel
    branch, the bucket of C) that tests/test_pointwise_layouts_gpu.py declares a case for."""
    declared = pw.declared_classes()
    n = 0
    for plan, seen in recorded.items():
        for name, calls in seen.items():
            if name in pw.ELSEWHERE:
                continue
            classes = {pw.point_class(name, d if isinstance(d, tuple) else (d,)) for d in calls}
            n += len(calls)
            missing = sorted((c for c in classes if not pw.class_covered(c, declared)), key=str)
            assert not missing, (plan, name, missing)
    assert n > 100, n
    kinds = {c[0] for plan, seen in recorded.items() for name, calls in seen.items() if name == "v1_op" for c in [pw.point_class(name, (d,)) for d in calls]}
    assert kinds == {"resize_aa", "sh_embed", "softmax", "attn_fewq", "head_mix", "add", "copy_rows", "camera_v1", "mean3", "preprocess_v1", "vit_tap",
                     "resize_ac_split", "out_conv3"}, kinds               # every V1 kind a plan records (POINTS runs outside the program)


def test_dispatch_branches_no_plan_records_are_declared_too():
    """finalize in both modes and the kernel branches no dry run reaches (the generic up-sampling kernel's shuffle and wide-LDS paths,
    ln_patchify2<4> / <8>, the 20-register softmax, the fp32 softmax) are in the declared set whether or not a plan records them."""
    declared = pw.declared_classes()
    missing = sorted((c for c in pw.REQUIRED_CLASSES if not pw.class_covered(c, declared)), key=str)
    assert not missing, missing
    ids = {c["id"] for c in pw.POINTWISE_CASES}
    assert {"softmax-reg20_N5120", "upsample2x-lds_C96", "upsample2x-lds_C512"} <= ids
    # one second-trip case per capped grid
    assert {c["op"] for c in pw.POINTWISE_CASES if "second_trip" in c["id"]} >= {"add", "mean3", "vit_tap", "copy_rows", "rays", "max", "upsample2x", "resize_ac",
                                                                                 "resize_ac_split", "resize_aa", "finalize", "preprocess_v1", "patchify4",
                                                                                 "head_mix", "points"}
    assert all(c["op"] in pw.OPS for c in pw.POINTWISE_CASES) and set(pw.OPS) == {c["op"] for c in pw.POINTWISE_CASES}
