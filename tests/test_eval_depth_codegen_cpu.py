"""Build-time guard of the 2-D depth metrics' reproducibility rule (csrc/evaldepth.hip): float sums are per-block partials reduced in a
fixed order, never float atomics.  The gfx950 device assembly (hipcc cross-compiles without a GPU) must hold no floating-point global
atomic; the integer counters and histograms are the only atomics."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "unidepth_amd", "csrc", "evaldepth.hip")


def test_no_float_atomics_in_eval_depth_kernels():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "evaldepth.s")
        flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result", "-ffp-contract=off"]
        subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", SRC, "-o", out], check=True, capture_output=True, timeout=600)
        asm = open(out).read()
    atomics = set(re.findall(r"\b(global_atomic_\w+|flat_atomic_\w+|buffer_atomic_\w+)", asm))
    assert atomics, "expected the integer counter atomics"
    assert not [a for a in atomics if re.search(r"f32|f64|fmin|fmax|cmpswap", a)], atomics
    assert "ed_stats_kernel" in asm and "ed_rescale_kernel" in asm
