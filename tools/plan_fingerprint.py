"""Fingerprints of the recorded launch programs (tests/golden/plan_fingerprints.json, checked by tests/test_plan_fingerprint_cpu.py).

A plan is built on the host (tests/dry_run.py: host tensors stand in for the device buffers, nothing runs) while every
`ud_program_add_*` call is logged.  The fingerprint of the plan is that stream, in order:

* the entry point and every scalar argument / descriptor field by value (nested structs and arrays field by field);
* every pointer by a canonical name instead of its address: `w:<key>+<byte offset>` for a packed weight, otherwise
  `b<ordinal>+<byte offset>/<allocation bytes>:<dtype>` with the ordinal counted in order of first use in the stream -- aliasing shows as
  offsets into one allocation, an undersized buffer as a changed size, and the order in which buffers are allocated does not matter;
* `prog.meta` (kernel class, tag, algorithmic flops and bytes per op), the `(name, position)` pairs of `tap_points` and the plan's
  shape-policy attributes.

Buffer lifetime is checked on the way: `torch.zeros` / `torch.empty` results are held until the build is over (no address can be reused),
and every non-weight pointer of the stream must fall inside a tensor reachable from `prog.keep` or the plan's attributes.

The golden file stores per signature the op count, one SHA-256 over the whole stream and one line per op (`index entry-point tag hash`),
so a mismatch names the first differing launch.  A pull request that leaves the launch programs alone (a refactor of the builders) must
leave the golden file byte-identical; one that changes a launch program on purpose regenerates it with

    python tools/plan_fingerprint.py --write

and shows the per-op diff of the golden file in review."""
import argparse
import bisect
import ctypes as C
import hashlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")
_spec = importlib.util.spec_from_file_location("dry_run", os.path.join(ROOT, "tests", "dry_run.py"))
dry_run = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dry_run)

ENTRY_POINTS = ("gemm layernorm row_stats_finalize attention linear_f32 camera_head attention_small_f32 preprocess fill_rows camera_intrinsics "
                "rays rays_camera ray_embed upsample2x resize_ac finalize nhwc_to_nchw dwconv7 layernorm_patchify2 patchify4 max spatial_mean "
                "v1_op").split()
V2_ATTRS = ("enc_first", "enc_last", "dec_first", "ln_fold", "cam_one_launch", "nb", "Hn", "Wn", "Ho", "Wo", "paddings", "rf")
V1_ATTRS = ("dec_first", "ratio", "pads")


class _Ptr(int):
    """A raw address in the logged stream, named once the build is over."""


def _struct(s):
    out = []
    for name, tp in s._fields_:
        v = getattr(s, name)
        if tp is C.c_void_p:
            out.append([name, _Ptr(v or 0)])
        elif isinstance(v, C.Array):
            out.append([name, [_struct(e) if isinstance(e, C.Structure) else e for e in v]])
        elif isinstance(v, C.Structure):
            out.append([name, _struct(v)])
        else:
            out.append([name, v])
    return out


def _tensors(obj, seen):
    """Every tensor reachable from `obj` through lists, tuples, dicts and object attributes (plan -> prog.keep, plan.enc -> ...)."""
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (list, tuple, set)):
        for v in obj:
            yield from _tensors(v, seen)
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v, seen)
    elif hasattr(obj, "__dict__") and not callable(obj):
        yield from _tensors(vars(obj), seen)


class _Ranges:
    """Address ranges -> names; later `add` calls do not replace earlier ones that start at the same address."""

    def __init__(self):
        self.starts, self.items = [], {}

    def add(self, start, nbytes, name):
        if nbytes and start not in self.items:
            bisect.insort(self.starts, start)
            self.items[start] = (nbytes, name)

    def find(self, p):
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0 and p < self.starts[i] + self.items[self.starts[i]][0]:
            return self.starts[i], self.items[self.starts[i]][1]
        return None


def _storage(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.nbytes(), str((t._base if t._base is not None else t).dtype).replace("torch.", "")


def record(model, build, attrs):
    """Build a plan with `build()` under the host dry run and return its fingerprint: dict(ops=count, sha256=..., lines=[...])."""
    from unidepth_amd import _lib
    stream, held = [], []

    def log(name):
        types = getattr(_lib.lib, "ud_program_add_" + name).argtypes

        def call(real, *args):
            row = []
            for a, tp in list(zip(args, types))[1:]:                      # args[0] is the program handle
                if tp is C.c_void_p:
                    row.append(_Ptr(a or 0))
                elif hasattr(a, "_obj"):
                    row.append(_struct(a._obj))
                else:
                    row.append(a)
            stream.append(("ud_program_add_" + name, row))
            return real(*args)
        return call

    real_alloc = {n: getattr(torch, n) for n in ("zeros", "empty")}

    def holding(fn):
        def alloc(*a, **kw):
            t = fn(*a, **kw)
            held.append(t)
            return t
        return alloc
    for n, fn in real_alloc.items():
        setattr(torch, n, holding(fn))
    try:
        with dry_run.host_recording({n: log(n) for n in ENTRY_POINTS}):
            plan = build()
    finally:
        for n, fn in real_alloc.items():
            setattr(torch, n, fn)

    weights, live, dead = _Ranges(), _Ranges(), _Ranges()
    for key in sorted(k for k, v in model._w.items() if torch.is_tensor(v)):
        start, nbytes, _ = _storage(model._w[key])
        weights.add(start, nbytes, key)
    for t in _tensors(plan, set()):
        start, nbytes, dtype = _storage(t)
        live.add(start, nbytes, (nbytes, dtype))
    for t in held:
        start, nbytes, dtype = _storage(t)
        dead.add(start, nbytes, (nbytes, dtype))
    ordinal, lost = {}, []

    def name_of(p, at):
        if not p:
            return "null"
        hit = weights.find(p)
        if hit:
            return "w:%s+%d" % (hit[1], p - hit[0])
        hit = live.find(p)
        if not hit:
            lost.append((at, stream[at][0], hex(p), dead.find(p)))
            return "lost"
        n = ordinal.setdefault(hit[0], len(ordinal))
        return "b%d+%d/%d:%s" % (n, p - hit[0], *hit[1])

    def canon(v, at):
        if isinstance(v, _Ptr):
            return name_of(int(v), at)
        if isinstance(v, (list, tuple)):
            return [canon(e, at) for e in v]
        return repr(v) if isinstance(v, float) else v

    meta = [list(m) for m in plan.prog.meta]
    assert len(meta) == len(stream) == len(plan.prog), (len(meta), len(stream), len(plan.prog))
    ops_c = [[name, canon(row, i), canon(meta[i], i)] for i, (name, row) in enumerate(stream)]
    assert not lost, "launches point into buffers the plan does not keep alive (op, entry point, address, allocation): %r" % lost[:5]
    lines = ["%d %s %s %s" % (i, o[0], o[2][1], hashlib.sha256(json.dumps(o).encode()).hexdigest()[:8]) for i, o in enumerate(ops_c)]
    taps = [[n, at] for n, at, _ in plan.tap_points]
    blob = json.dumps([ops_c, taps, [[a, canon(getattr(plan, a), 0)] for a in attrs]])
    return dict(ops=len(ops_c), sha256=hashlib.sha256(blob.encode()).hexdigest(), lines=lines)


# ---- the pinned signatures: (name, model key, set-up, build)
def _v2(*a, **kw):
    return lambda m: m._plan(*a, **kw)


def _no_camera_head(build):
    def run(m):
        from unidepth_amd import ops
        real = ops.camera_head_supported
        ops.camera_head_supported = lambda d: False
        try:
            return build(m)
        finally:
            ops.camera_head_supported = real
    return run


def _ln_fold_off(build):
    def run(m):
        m.ln_fold_force = False
        try:
            return build(m)
        finally:
            del m.ln_fold_force
    return run


def _level(level, build):
    def run(m):
        old, m.resolution_level = m.resolution_level, level
        try:
            return build(m)
        finally:
            m.resolution_level = old
    return run


MODELS = {
    "v2.vits14": lambda: dry_run.v2_model("vits14", 3, 2),
    "v2.vitl14": lambda: dry_run.v2_model("vitl14", 3, 2),
    "v1.cnvnxtl": lambda: dry_run.v1_model("cnvnxtl", 301),
    "v1.vitl14": lambda: dry_run.v1_model("vitl14", 301),
}
_V1_DEFAULT = (1, 240, 320, True, False, True, 0, False)
SIGNATURES = [
    ("v2.vits14/b1_462x616_u8", _v2(1, 462, 616, 0, True, True)),
    ("v2.vits14/b1_462x616_u8_per_layer_camera_head", _no_camera_head(_v2(1, 462, 616, 0, True, True))),
    ("v2.vits14/b2_462x616_pinhole_broadcast", _v2(2, 462, 616, 1, False, True, gt_mode=1)),
    ("v2.vits14/b2_462x616_closed_form_per_image", _v2(2, 462, 616, 2, False, True, gt_mode=2)),
    ("v2.vits14/b2_462x616_iterative_model", _v2(2, 462, 616, 1, False, True, gt_mode=4)),
    ("v2.vits14/b2_462x616_mixed_batch_camera", _v2(2, 462, 616, 2, False, True, gt_mode=(1, 5))),
    ("v2.vits14/b1_462x616_seam_given_rays", _v2(1, 462, 616, 1, False, False, gt_mode=15, net=True)),
    ("v2.vits14/b1_462x616_seam", _v2(1, 462, 616, 0, False, False, net=True)),
    ("v2.vitl14/b8_518x518_seam_ln_fold", _v2(8, 518, 518, 0, False, False, net=True)),
    ("v2.vitl14/b8_518x518_seam_ln_fold_off", _ln_fold_off(_v2(8, 518, 518, 0, False, False, net=True))),
    ("v2.vitl14/b1_518x518_u8_level9", _level(9, _v2(1, 518, 518, 0, True, True))),
    ("v1.cnvnxtl/full_b1_240x320_u8", lambda m: m._full_plan(*_V1_DEFAULT)),
    ("v1.cnvnxtl/full_b2_240x320_one_gt_camera", lambda m: m._full_plan(2, 240, 320, False, False, True, 1, False)),
    ("v1.cnvnxtl/full_b2_240x320_skip_camera", lambda m: m._full_plan(2, 240, 320, True, False, True, 2, True)),
    ("v1.cnvnxtl/enc_b1_224x320", lambda m: m._enc_plan(1, 224, 320)),
    ("v1.vitl14/full_b1_240x320_u8", lambda m: m._full_plan(*_V1_DEFAULT)),
    ("v1.vitl14/enc_b1_224x308", lambda m: m._enc_plan(1, 224, 308)),
]


def fingerprint(model, name, build):
    """Fingerprint of one pinned signature on `model` (one of MODELS); the plan cache is cleared first and afterwards."""
    attrs = V2_ATTRS if name.startswith("v2.") else V1_ATTRS if "/full_" in name else ()
    model.clear_plans()
    try:
        return record(model, lambda: build(model), attrs)
    finally:
        model.clear_plans()


def all_fingerprints():
    out, models = {}, {}
    for name, build in SIGNATURES:
        key = name.split("/")[0]
        if key not in models:
            models.clear()                                                  # one synthetic model in memory at a time
            models[key] = MODELS[key]()
        out[name] = fingerprint(models[key], name, build)
    return out


def first_difference(got, want):
    """None if the two fingerprints agree, otherwise a line that names the first differing launch."""
    if got == want:
        return None
    for i, (a, b) in enumerate(zip(got["lines"], want["lines"])):
        if a != b:
            return "op %d: recorded %r, golden %r" % (i, a, b)
    if got["ops"] != want["ops"]:
        return "%d ops recorded, %d in the golden file (the first %d agree)" % (got["ops"], want["ops"], min(got["ops"], want["ops"]))
    return "every launch agrees; tap points or plan attributes differ (sha256 %s, golden %s)" % (got["sha256"][:12], want["sha256"][:12])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate tests/golden/plan_fingerprints.json (a launch program changed on purpose)")
    args = ap.parse_args()
    got = all_fingerprints()
    if args.write:
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
        return 0
    with open(GOLDEN) as f:
        want = json.load(f)
    bad = 0
    for name in sorted(set(got) | set(want)):
        diff = "missing" if name not in got or name not in want else first_difference(got[name], want[name])
        print("%-60s %5s ops  %s" % (name, got.get(name, {}).get("ops", "-"), diff or "ok"))
        bad += diff is not None
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
