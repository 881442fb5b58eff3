"""The host programs of the camera-map tests (not a test module): tests/<name>/<name>.cpp compiles a header of unidepth_amd/csrc for the
CPU into a stand-alone program with its own main, which reads its inputs from stdin and writes its outputs to stdout.  One compiler line,
one way to run such a program, and the bit comparisons the tests of those outputs share."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# -ffp-contract=off: no fused multiply-adds, the rounding the .hip files of these headers are built with
FLAGS = ["-O2", "-ffp-contract=off"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(tmp_path_factory, name, sanitize=True):
    """tests/<name>/<name>.cpp -> the path of the program, under AddressSanitizer and UBSan unless sanitize=False"""
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++"] + FLAGS + (SANITIZE if sanitize else []) + ["-o", out, os.path.join(ROOT, "tests", name, name + ".cpp")])
    return out


def run(exe, args, blobs, sizes):
    """exe with str(args) on its command line and the blobs on stdin; it must exit with 0 (the failure shows the end of stderr: the
    program's own complaint or a sanitizer's report) and write sum(sizes) bytes -> those bytes cut into len(sizes) slices"""
    p = subprocess.run([exe] + [str(a) for a in args], input=b"".join(blobs), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    assert len(p.stdout) == sum(sizes), (len(p.stdout), sizes)
    at = np.cumsum([0] + list(sizes))
    return [p.stdout[at[k]:at[k + 1]] for k in range(len(sizes))]


def f32_bits(v):
    """the bit pattern of v rounded to fp32, as the descriptors and the programs' command lines carry a tolerance"""
    return struct.unpack("<i", struct.pack("<f", v))[0]


def same_bits(a, b):
    """numpy arrays equal in shape, dtype and every bit: NaN payloads and the sign of a zero count"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bits(t):
    """a tensor as integers of its element width: NaN payloads and the sign of a zero count"""
    import torch
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8) if t.dtype == torch.bool else t


def assert_same(got, want, names, what=""):
    """tuples of tensors (or None, on both sides): every output, every element, bit for bit; the message says which output, how many
    elements and the first of them"""
    import torch
    assert len(got) == len(want) == len(names), (what, len(got), len(want))
    for name, a, b in zip(names, got, want):
        assert (a is None) == (b is None), (what, name)
        if a is None:
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        if not torch.equal(bits(a), bits(b)):
            diff = (bits(a) != bits(b)).reshape(-1)
            both_nan = ((a != a) & (b != b)).reshape(-1) if a.is_floating_point() else torch.zeros_like(diff)
            raise AssertionError(f"{what}: {name} differs in {int(diff.sum())} of {diff.numel()} elements ({int((diff & both_nan).sum())} of "
                                 f"them NaN on both sides), first at flat index {int(diff.nonzero()[0])}: "
                                 f"{a.reshape(-1)[diff][:4].tolist()} vs {b.reshape(-1)[diff][:4].tolist()}")
