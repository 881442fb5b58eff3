"""Host dry run of the plan builders: a launch program is RECORDED with host tensors standing in for the device buffers, nothing runs.
One harness for the tests that do this (test_host_cpu, test_layout_coverage_cpu, test_plan_fingerprint_cpu) and for
tools/plan_fingerprint.py.  A plain helper module, not a conftest."""
import contextlib

import torch


@contextlib.contextmanager
def host_recording(intercept=None):
    """Inside the block `torch.cuda.device` is a no-op context, `ops.ptr` accepts host tensors, and every `ud_program_add_<name>` entry
    point named in `intercept` ({name: fn(real, *args) -> return code}) goes through its `fn` (which calls `real(*args)` itself)."""
    from unidepth_amd import _lib, ops
    saved = [(torch.cuda, "device", torch.cuda.device), (ops, "ptr", ops.ptr)]
    torch.cuda.device = lambda d: contextlib.nullcontext()
    ops.ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    for name, fn in (intercept or {}).items():
        real = getattr(_lib.lib, "ud_program_add_" + name)
        saved.append((ops.lib, "ud_program_add_" + name, real))
        setattr(ops.lib, "ud_program_add_" + name, lambda *a, fn=fn, real=real: fn(real, *a))
    try:
        yield
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)


def v2_model(arch="vits14", seed=3, resolution_level=2):
    """A UniDepthV2 on a synthetic checkpoint with host-packed weights (device = cpu: plans can be recorded, nothing can run)."""
    from oracle import synth
    from unidepth_amd import UniDepthV2
    from unidepth_amd.weights import pack
    cfg = synth.load_config(arch)
    m = UniDepthV2(cfg).load_state_dict(synth.make_synthetic_checkpoint(cfg, seed))
    dev = torch.device("cpu")
    m._w = pack(cfg, m._sd, dev)
    m._device = dev
    m.resolution_level = resolution_level
    return m


def v1_model(arch="cnvnxtl", seed=301):
    """A UniDepthV1 (ConvNeXt-L or ViT-L backbone) on a synthetic checkpoint with host-packed weights."""
    from oracle import synth_v1
    from unidepth_amd import UniDepthV1, unidepthv1 as U
    cfg = synth_v1.load_config_v1(arch)
    m = UniDepthV1(cfg).load_state_dict(synth_v1.make_synthetic_checkpoint_v1(cfg, seed))
    dev = torch.device("cpu")
    m._w = {**(U.pack_vit if m._arch["kind"] == "vit" else U.pack_convnext)(cfg, m._sd, dev), **U.pack_v1_decoder(cfg, m._sd, dev)}
    m._device = dev
    return m
