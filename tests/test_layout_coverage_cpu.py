"""The guarded-layout GPU matrices (tests/test_kernel_layouts_gpu.py, tests/test_pointwise_layouts_gpu.py) stay complete: every descriptor
that the launch programs of SIGNATURES record on the host -- through ANY ud_program_add_* entry point -- falls into a class one of the two
GPU modules covers, so a product path cannot appear without a guarded GPU test.  SIGNATURES holds the single-image plans and the batched
ones the benchmark, the parity tests and the golden cases run (V2 ViT-S / ViT-B / ViT-L up to batch 32, every resolution level and camera
model of oracle/cases.py; V1 ConvNeXt-L / ViT-L up to batch 16): tile selection, the LayerNorm fold, the grouped-as-one launch, the
row-balanced schedule and the dwconv7 branch all depend on M = B x tokens.  Nothing runs on a device: the plans are recorded with host
tensors standing in for the device buffers (the dry runs of tests/test_host_cpu.py), one signature at a time, and only the SETS of classes
are kept (a V1 plan at batch 16 holds ~10 GB of stand-ins)."""
import ctypes as C
import importlib.util
import os
import re
import warnings

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

_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "unidepth_hip.h")
ENTRY_POINTS = sorted(set(re.findall(r"ud_program_add_(\w+)\(", open(_HEADER).read())))      # every recording entry point of the C-ABI
_FLAGS = {"linear_f32": "linear_flags", "layernorm": "layernorm_flags", "attention": "attention_flags"}


def _v2(arch, B, H, W, level=2, cam_nb=0, gt_mode=0):
    """One UniDepthV2 signature: uint8 input, normalised; level None leaves resolution_level unset (the default pixel bounds of infer())."""
    return ("v2", arch, f"b{B}_{H}x{W}_lvl{level}_cam{cam_nb}m{gt_mode}", (B, H, W, cam_nb, True, True), dict(level=level, gt_mode=gt_mode))


def _v1(arch, B, H, W, n_gt=0, skip=False):
    return ("v1", arch, f"b{B}_{H}x{W}_gt{n_gt}_skip{skip:d}", (B, H, W, True, False, True, n_gt, skip), {})


# Every signature the coverage tests record, grouped by model (one synthetic model lives at a time).  The batched ones are what bench.py,
# the parity tests and the golden cases run: M = B x tokens moves the tile choice of route(), the LayerNorm fold, the grouped-as-one launch,
# the row-balanced schedule and the dwconv7 branch.
SIGNATURES = [
    # UniDepthV2 ViT-S/14: the demo shape, its batch of 8, and the shapes / camera models of oracle/cases.py
    _v2("vits14", 1, 462, 616), _v2("vits14", 8, 462, 616), _v2("vits14", 1, 462, 616, None), _v2("vits14", 2, 480, 640, None, 1, 1),
    _v2("vits14", 1, 375, 1242, None), _v2("vits14", 1, 300, 400, None, 1, 2), _v2("vits14", 2, 200, 560, None, 1, 3),
    _v2("vits14", 1, 300, 400, None, 1, 4), _v2("vits14", 1, 300, 400, None, 1, 5), _v2("vits14", 2, 200, 640, None, 1, 6),
    # ViT-B/14: a golden case
    _v2("vitb14", 1, 518, 518), _v2("vitb14", 8, 518, 518), _v2("vitb14", 1, 518, 518, None),
    # ViT-L/14: the headline benchmark (batch 8 at 518 x 518) and the batches of the scaling runs, the resolution levels, an iterative camera
    _v2("vitl14", 1, 462, 616), _v2("vitl14", 8, 518, 518), _v2("vitl14", 8, 518, 518, None), _v2("vitl14", 16, 518, 518), _v2("vitl14", 32, 518, 518),
    _v2("vitl14", 2, 644, 966, 3), _v2("vitl14", 1, 644, 966, 3), _v2("vitl14", 1, 518, 518, 9), _v2("vitl14", 1, 518, 518, 0),
    _v2("vitl14", 1, 518, 518, None), _v2("vitl14", 4, 518, 518, 2, 1, 6),
    # UniDepthV1 ConvNeXt-L: the golden shapes (with and without the given camera) and the benchmark's batch of 16 at 480 x 640
    _v1("cnvnxtl", 1, 240, 320), _v1("cnvnxtl", 1, 128, 160), _v1("cnvnxtl", 2, 200, 360), _v1("cnvnxtl", 2, 200, 360, 2, False),
    _v1("cnvnxtl", 2, 200, 360, 2, True), _v1("cnvnxtl", 1, 480, 640), _v1("cnvnxtl", 16, 480, 640),
    # UniDepthV1 ViT-L/14
    _v1("vitl14", 1, 240, 320), _v1("vitl14", 1, 200, 360, 1, False), _v1("vitl14", 8, 480, 640), _v1("vitl14", 16, 480, 640),
]


def _record(model, kind, sig, opts):
    """Every ud_program_add_* call of one plan, by entry point.  The plan (host stand-ins of its device buffers: gigabytes at the large
    batches) is dropped before this returns."""
    seen = {k: [] for k in ENTRY_POINTS}

    def log(name):
        def add(real, h, *a):
            # a descriptor struct is copied (the caller's goes out of scope); scalar argument lists are kept as they are
            seen[name].append(type(a[0]._obj).from_buffer_copy(a[0]._obj) if len(a) == 1 and hasattr(a[0], "_obj") else a)
            return real(h, *a)
        return add
    model.clear_plans()
    try:
        with dry_run.host_recording({name: log(name) for name in seen}):
            if kind == "v2":
                if opts["level"] is None:
                    if hasattr(model, "resolution_level"):
                        del model.resolution_level
                else:
                    model.resolution_level = opts["level"]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                       # "resolution_level not set": the signature means it
                    model._plan(*sig, gt_mode=opts["gt_mode"])
            else:
                model._full_plan(*sig)
    finally:
        model.clear_plans()
    return seen


def _classes(seen):
    """What the tests below read of one recording: the number of calls per entry point and the SETS of classes (no descriptor is kept)."""
    out = dict(count={name: len(calls) for name, calls in seen.items()}, gemm={lay.gemm_class(d) for d in seen["gemm"]})
    for op, flags in _FLAGS.items():
        out[op] = {getattr(lay, flags)(d) for d in seen[op]}
    out["attention_schedule"] = {lay.attention_schedule(d) for d in seen["attention"]}
    out["point"] = {name: {pw.point_class(name, d if isinstance(d, tuple) else (d,)) for d in calls}
                    for name, calls in seen.items() if name not in pw.ELSEWHERE}
    return out


def recordings(signatures=None):
    """(plan name, recorded calls by entry point) of every signature, one at a time; one synthetic model lives at a time."""
    model = key = None
    for kind, arch, tag, sig, opts in signatures or SIGNATURES:
        if key != (kind, arch):
            model = None                                                      # the previous model goes before the next is built
            key, model = (kind, arch), (dry_run.v2_model(arch, 3, 2) if kind == "v2" else dry_run.v1_model(arch, 301))
        yield f"{kind}/{arch}/{tag}", _record(model, kind, sig, opts)


@pytest.fixture(scope="module")
def recorded():
    if torch.cuda.is_available():
        pytest.skip("host-only dry run")
    out = {plan: _classes(seen) for plan, seen in recordings()}
    assert len(out) == len(SIGNATURES)
    return out


def test_gemm_cases_reach_the_schedule_they_name():
    """Each GPU case's descriptor, built on the host, picks the schedule the case declares -- at every layout it runs."""
    from unidepth_amd import _lib
    bad = [(c["id"], lo, _lib.lib.ud_gemm_pick(C.byref(lay.host_desc(c, lo)))) for c in lay.GEMM_CASES for lo in lay._lay(c)
           if _lib.lib.ud_gemm_pick(C.byref(lay.host_desc(c, lo))) != c["pick"]]
    assert not bad, bad
    picks = {c["pick"] for c in lay.GEMM_CASES}
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 19, 20, 24, 36} <= picks
    hints = {c.get("hint", 0) for c in lay.GEMM_CASES}
    assert {1, 2, 3, 5, 7, 8, 9, 10, 11, 12, 13, 14} <= hints           # every tile_hint of include/unidepth_hip.h (6: the auto ring cases)


def test_every_product_gemm_class_has_a_guarded_gpu_case(recorded):
    declared = lay.declared_gemm_classes()
    missing = {}
    for plan, seen in recorded.items():
        assert seen["count"]["gemm"] > 60, plan
        if seen["gemm"] - declared:
            missing[plan] = sorted(seen["gemm"] - declared)
    assert not missing, missing


@pytest.mark.parametrize("op,flags,table", [("linear_f32", "linear_flags", "LINEAR_F32_FLAGS"), ("layernorm", "layernorm_flags", "LAYERNORM_FLAGS"),
                                            ("attention", "attention_flags", "ATTENTION_FLAGS")])
def test_every_product_descriptor_stride_class_is_covered(recorded, op, flags, table):
    declared = getattr(lay, table)                # recorded[plan][op]: the set of lay.<flags>(descriptor) over the plan (_classes)
    assert _FLAGS[op] == flags
    missing = {}
    for plan, seen in recorded.items():
        # every plan records LayerNorm and attention launches; ud_linear_f32 is the V1 camera head's (skipped with skip_camera)
        assert seen["count"][op] > 0 or (op == "linear_f32" and (plan.startswith("v2/") or plan.endswith("_skip1"))), (plan, op)
        if seen[op] - declared:
            missing[plan] = sorted(seen[op] - declared)
    assert not missing, (op, missing)
    assert sum(seen["count"][op] for seen in recorded.values()) > 0, op


def test_every_product_attention_schedule_has_a_guarded_gpu_case(recorded):
    """Every attention descriptor of the recorded plans falls into a schedule class (lay.attention_schedule: kernel, steady loop, the tiles
    after it, key tail, persistent walk, fewer pairs than XCDs) that a case of ATT_CASES or of tests/test_attention_paths_gpu.py runs."""
    missing = {plan: sorted(seen["attention_schedule"] - lay.ATTENTION_SCHEDULES, key=str) for plan, seen in recorded.items()
               if seen["attention_schedule"] - lay.ATTENTION_SCHEDULES}
    assert not missing, missing
    assert all(seen["attention_schedule"] for seen in recorded.values())


def test_attention_schedule_branches_no_plan_needs_are_declared_too():
    """The tile-count branches of attention_pipe_kernel that no randn case of the suite ran before tests/test_attention_paths_gpu.py: each is
    named here, so dropping the group of cases that reaches it fails this test by name."""
    have = lay.ATTENTION_SCHEDULES
    want = {"one tile with a tail (nt == 1 && tail)": ("pipe", False, 1, True, False, True),
            "rem == 3 without the steady loop (nt = 3)": ("pipe", False, 3, True, False, True),
            "nt = 6: the steady loop twice, rem 2": ("pipe", True, 2, True, False, True),
            "nt = 7: the steady loop twice, rem 3": ("pipe", True, 3, True, False, True),
            "a single-tile item with a successor": ("pipe", False, 1, True, True, False),
            "fewer pairs than XCDs, no tail": ("pipe", False, 1, False, False, True),
            "one-tile kernel, one tile with a tail": ("tile", True, True),
            "one-tile kernel, several tiles, no tail": ("tile", False, False)}
    missing = sorted(name for name, cls in want.items() if cls not in have)
    assert not missing, missing
    nts = {(c["pre"], -(-c["Nk"] // 64), c["Nk"] % 64 != 0) for c in lay.att_paths.CASES if c["B"] * c["H"] < 8}
    assert {(pre, nt, tail) for pre in (0, 1) for nt in range(1, 8) for tail in (False, True)} <= nts      # the class does not tell nt = 6 from 4
    walks = [lay._attention_schedule(c["B"], c["H"], c["Nq"], c["Nk"], True)[4] for c in lay.att_paths.CASES if c["group"] == "d"]
    assert walks and all(walks)                                                                            # the persistent-walk cases walk


def test_every_entry_point_is_intercepted(recorded):
    assert len(ENTRY_POINTS) == 23 and {"gemm", "v1_op", "fill_rows", "dwconv7", "finalize"} <= set(ENTRY_POINTS)
    used = {name for seen in recorded.values() for name, n in seen["count"].items() if n}
    assert {"fill_rows", "camera_intrinsics", "rays", "ray_embed", "upsample2x", "resize_ac", "nhwc_to_nchw", "dwconv7", "layernorm_patchify2", "patchify4",
            "spatial_mean", "attention_small_f32", "v1_op"} <= used, used


def test_every_product_pointwise_class_has_a_guarded_gpu_case(recorded):
    """Every recorded descriptor outside the GEMM / LayerNorm / attention family maps to a class (op or V1 kind, the flags that pick a kernel
    branch, the bucket of C) that tests/test_pointwise_layouts_gpu.py declares a case for."""
    declared = pw.declared_classes()
    missing, n = {}, 0
    for plan, seen in recorded.items():
        n_plan = sum(seen["count"][name] for name in seen["point"])
        assert n_plan > 0, plan
        n += n_plan
        for name, classes in seen["point"].items():
            bad = sorted((c for c in classes if not pw.class_covered(c, declared)), key=str)
            if bad:
                missing[plan, name] = bad
    assert not missing, missing
    assert n > 100, n
    kinds = {c[0] for seen in recorded.values() for c in seen["point"]["v1_op"]}
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
