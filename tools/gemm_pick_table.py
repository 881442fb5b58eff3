"""The GEMM route decision, pinned (tests/golden/gemm_pick_table.json, checked by tests/test_gemm_pick_table_cpu.py).

`route()` in csrc/gemm.hip decides which schedule and which kernel instantiation a UdGemm descriptor runs on; `ud_gemm_pick` and
`ud_gemm_kernel_name` report that decision without launching anything (host code: it reads the scalar fields and which pointers are set).
The table lists descriptors -- a grid over shapes, epilogues, A modes, hints and flag fields, the cases of the guarded GPU matrix
(tests/test_kernel_layouts_gpu.py GEMM_CASES) and every GEMM descriptor of the three dry-run plans of tests/test_layout_coverage_cpu.py --
each with the pick value and the kernel class label.  A row stores only what differs from the defaults of `desc()` below.

    python tools/gemm_pick_table.py            compare the library's answers with the table
    python tools/gemm_pick_table.py --write    regenerate the table (the decision changed on purpose; show the diff in review)
    python tools/gemm_pick_table.py --sweep [--lib PATH]
                                               ud_gemm_pick over a product grid of 13.8 million descriptors, one SHA-256 per chunk and
                                               one over all: two builds of the library decide alike iff the digests agree"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_pick_table.json")
PLANS = (("v2", "vits14"), ("v2", "vitl14"), ("v1", "cnvnxtl"))
MNK = ("M", "N", "K")     # stored by position in a table row
DUMMY = 0x10000           # placeholder address: the decision only tests pointers against null


def _tests_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fields():
    from unidepth_amd import _lib
    ptrs = [n for n, t in _lib.UdGemm._fields_ if t is C.c_void_p]
    return ptrs, [n for n, t in _lib.UdGemm._fields_ if t is not C.c_void_p and n != "grp_rows"]


def _defaults(d):
    """Field values a row need not spell out (derived from the fields it does)."""
    dv = dict(A=1, W=1, out=1, bias=1, lda=d.K, ldw=d.K, ldc=d.N)
    if d.amode:
        dv.update(zeros=1, cstride=d.Cin, rows_img=d.Himg * d.Wimg, img_stride=d.rows_img * d.cstride)
    return dv


def desc(row):
    """UdGemm of a table row: the row's fields, then the defaults above, every other field 0 / null.  Pointers are 1 (set) / 0 (null)."""
    from unidepth_amd import _lib
    ptrs, _ = _fields()
    d = _lib.UdGemm()
    for k, v in row.items():
        setattr(d, k, (DUMMY if v else None) if k in ptrs else v)
    for k in ("lda", "ldw", "ldc", "cstride", "rows_img", "img_stride", "A", "W", "out", "bias", "zeros"):     # in dependency order
        if k not in row and k in _defaults(d):
            v = _defaults(d)[k]
            setattr(d, k, (DUMMY if v else None) if k in ptrs else v)
    return d


def row_of(d):
    """The table row of a recorded descriptor: scalar fields by value, pointers as set / null; defaults left out."""
    ptrs, scalars = _fields()
    dv = _defaults(d)
    row = {k: (int(bool(getattr(d, k))) if k in ptrs else getattr(d, k)) for k in ptrs + scalars}
    return {k: v for k, v in row.items() if v != dv.get(k, 0) or k in MNK}


def answer(lib, d):
    buf = C.create_string_buffer(96)
    rc = lib.ud_gemm_kernel_name(C.byref(d), buf, len(buf))
    assert rc == 0, rc
    return lib.ud_gemm_pick(C.byref(d)), buf.value.decode()


# ---- the descriptors -------------------------------------------------------------------------------------------------------------------
def grid_rows():
    """Descriptors ud_gemm_f16 accepts (its argument checks: include/unidepth_hip.h).  A row with `large` set (popped by build_table) is one the
    checks accept only where the tile-shape model gives the problem to the large-tile kernels; it is dropped elsewhere."""
    rows = []
    F16, F32, QKV, D2S, HEAD = range(5)

    def add(hint=0, **r):
        if hint:
            r["tile_hint"] = hint
        if r.get("epi", 0) == QKV:
            r.update(out2=1, vsplit=r["N"] // 3 * 2 // 128 * 128)      # (of the epilogue geometry, the decision reads vsplit only)
        rows.append(r)

    # dense shapes x epilogue x every hint value 0..15 (4 and 15 are unassigned: whatever the library answers is recorded)
    shapes = [(256, 256, 1024), (1370, 384, 384), (1370, 1152, 384), (4096, 1024, 1024), (4096, 1024, 4096), (11008, 1024, 1024), (11008, 4096, 1024),
              (11008, 3072, 1024), (5480, 256, 2048), (21904, 256, 256), (8192, 192, 128), (3000, 64, 256), (3000, 32, 128)]
    for (M, N, K), epi, hint in itertools.product(shapes, (F16, F32, QKV, D2S), range(16)):
        if epi != QKV or N > 64:
            add(hint, M=M, N=N, K=K, epi=epi)
    # flag fields, each with and without, on shapes that reach the small, the ring and the large-tile schedules
    both = [dict(), dict(groups=4), dict(a_wrap=-2), dict(w_wrap=-2), dict(splitk_ws=1, splitk_cnt=1), dict(splitk_ws=1, splitk_cnt=1, splitk_ws_bytes=1 << 26),
            dict(add=1, ldadd=1024), dict(rows_in=137, rows_out=140), dict(act=1), dict(out2=1, act2=2, ldc2=1024)]
    flags = {F16: both + [dict(row_stats_in=1, wsum=1, large=1)],
             F32: both + [dict(accumulate=1), dict(accumulate=2, out2=1), dict(max_out=1, max_init=1), dict(row_stats_out=1, out2=1),
                          dict(row_stats_out=1, row_stats_final=1, row_stats_ticket=1, ln_D=1024, out2=1, large=1)]}
    for (M, N, K), epi, hint in itertools.product([(256, 1024, 1024), (1370, 1024, 2048), (5480, 1024, 4096), (11008, 4096, 1024), (11008, 1024, 1024)],
                                                  (F16, F32), (0, 3, 8, 10, 11)):
        for fl in flags[epi]:
            if "row_stats_final" in fl and N > 1024:         # (the in-kernel reduction takes rows of at most 1024 columns)
                continue
            r = dict(M=M, N=N, K=K, epi=epi, **{k: (K // 2 if v == -2 else v) for k, v in fl.items()})
            if fl.get("groups"):
                r.update(gW=N * K, gBias=N, gOut=M * N)
            add(hint, **r)
    # folded-LayerNorm consumers of both fp16 epilogues on every large-tile schedule
    for (M, N, K), epi, hint in itertools.product([(11008, 3072, 1024), (11008, 4096, 1024), (2740, 3072, 1024)], (F16, QKV), (0, 2, 3, 8, 9)):
        add(hint, M=M, N=N, K=K, epi=epi, row_stats_in=1, wsum=1, large=1)
    # grouped problems: shared / stacked A, fp16 / fp32 / QKV epilogues
    for M, gA, (epi, acc), K, hint in itertools.product((1024, 5632), (0, 1), ((F16, 0), (F32, 0), (F32, 1), (QKV, 0)), (256, 1024), (0, 1, 2)):
        r = dict(M=M, N=1024 if epi != QKV else 1536, K=K, epi=epi, accumulate=acc, groups=4, gA=gA * M * K, gW=1024 * K, gBias=1024, gOut=M * 1024)
        if epi == QKV:
            r.update(gOut=M * 1536, tok_per_img=M // 4, kv_ld=M // 4, heads_v=8, gOut2=4 * 8 * 64 * (M // 4))
        add(hint, **r)
    # 3x3 convolutions: every A mode with the epilogues it has, narrow and wide outputs
    for (amode, epi), N, Cin, (H, W), hint in itertools.product(((1, F16), (1, F32), (2, F16), (2, HEAD), (3, HEAD)), (32, 64, 256), (64, 128),
                                                                ((16, 16), (74, 74), (128, 160)), (0, 1, 2, 3, 8)):
        if (epi == HEAD and N != 32) or (amode == 3 and hint == 1):      # (the fused up-sampling exists in the halo-tile kernels only)
            continue
        r = dict(amode=amode, Himg=H, Wimg=W, Cin=Cin, M=2 * H * W, N=N, K=9 * Cin, epi=epi)
        if epi == HEAD:
            r.update(w2=1)
        if amode == 3:
            r.update(Hsrc=H // 2, Wsrc=W // 2)
        add(hint, **r)
    for H, Cin, spl in itertools.product((64, 96, 148), (256, 512), (0, 1)):       # the decoder's stage-0 convolutions: large-tile K split
        r = dict(amode=1, Himg=H, Wimg=H, Cin=Cin, M=H * H, N=Cin, K=9 * Cin, epi=F32, accumulate=1)
        if spl:
            r.update(splitk_ws=1, splitk_cnt=1, splitk_ws_bytes=1 << 26)
        add(**r)
    return rows


def case_rows():
    lay = _tests_module("test_kernel_layouts_gpu")
    return [row_of(lay.host_desc(c, lo)) for c in lay.GEMM_CASES for lo in lay._lay(c)]


def plan_rows():
    """Every GEMM descriptor the three dry-run plans record (tests/test_layout_coverage_cpu.py), by scalar fields."""
    dry_run = _tests_module("dry_run")
    rows = []

    def add(real, h, dref):
        rows.append(row_of(dref._obj))
        return real(h, dref)
    with dry_run.host_recording({"gemm": add}):
        for kind, arch in PLANS:
            if kind == "v2":
                dry_run.v2_model(arch, 3, 2)._plan(1, 462, 616, 0, True, True)
            else:
                dry_run.v1_model(arch, 301)._full_plan(1, 240, 320, True, False, True, 0, False)
    return rows


def key(row):
    return json.dumps(row, sort_keys=True)


def build_table(lib):
    rows, seen = [], set()
    for r in grid_rows() + case_rows() + plan_rows():
        if key(r) not in seen:
            seen.add(key(r))
            rows.append(r)
    table = {}                            # kernel class label -> its rows, [pick, M, N, K, {the other fields}]
    for r in rows:
        large = r.pop("large", 0)
        pick, label = answer(lib, desc(r))
        if large and pick & 15 not in (3, 4, 8):
            continue
        table.setdefault(label, []).append([pick] + [r[k] for k in MNK] + [{k: v for k, v in r.items() if k not in MNK}])
    return table


def table_rows(table):
    """(row dict, pick, label) of every row of a table as stored."""
    for label, rows in table.items():
        for pick, M, N, K, rest in rows:
            yield dict(rest, M=M, N=N, K=K), pick, label


def write_table(table, path):
    with open(path, "w") as f:            # one row per line under its label: a change of the decision shows as a line diff
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(label), ",\n".join(json.dumps(r, separators=(",", ":"), sort_keys=True) for r in table[label]))
                                   for label in sorted(table)) + "\n}\n")


# ---- the wide sweep --------------------------------------------------------------------------------------------------------------------
def sweep(lib):
    """ud_gemm_pick over the product grid below; prints one digest per (epi, amode) chunk and one over all."""
    from unidepth_amd import _lib
    Ms = (64, 256, 1000, 1024, 1370, 2740, 4096, 5480, 8192, 11008, 21904, 44032)
    Ns = (32, 64, 128, 192, 256, 384, 1024, 1536, 3072, 4096)
    Ks = (64, 128, 256, 1024, 2048, 4096)
    hints = range(16)
    groups = (0, 4)
    scratch = ((0, 0), (1, 0), (1, 1 << 28))
    flag_sets = (dict(), dict(accumulate=1), dict(row_stats_in=DUMMY, wsum=DUMMY), dict(row_stats_out=DUMMY), dict(row_stats_out=DUMMY, row_stats_final=DUMMY, row_stats_ticket=DUMMY, ln_D=1024),
                 dict(max_out=DUMMY), dict(a_wrap=64), dict(w_wrap=64), dict(add=DUMMY, rows_in=100), dict(act=1, out2=DUMMY))
    flag_names = sorted({k for f in flag_sets for k in f})
    total, n = hashlib.sha256(), 0
    pick = lib.ud_gemm_pick
    print("grid: M %s x N %s x K %s x hint 0..15 x groups %s x scratch (none, small, small + large) x %d flag sets, per (epi, amode)" % (Ms, Ns, Ks, groups, len(flag_sets)))
    for epi, amode in itertools.product(range(5), range(4)):
        d = _lib.UdGemm()
        d.A = d.W = d.out = d.bias = d.zeros = d.w2 = DUMMY
        d.epi, d.amode = epi, amode
        d.out2 = DUMMY if epi == 2 else None
        d.vsplit, d.heads_v = 1024, 8
        d.d2s_k, d.d2s_Co = 2, 8
        d.Hsrc = d.Wsrc = 8
        ref = C.byref(d)
        out = bytearray()
        for M, N, K in itertools.product(Ms, Ns, Ks):
            d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.ldc2 = M, N, K, K, K, N, N
            d.tok_per_img = d.kv_ld = M // 4 if M % 16 == 0 else M
            if amode:                      # valid conv geometry: M = 4 images of H x W pixels (H * W = M / 4 where that divides), K = 9 * Cin
                hw = M // 4
                H = next(h for h in (148, 128, 74, 64, 37, 32, 25, 16, 10, 8, 5, 4, 2, 1) if hw % h == 0)
                d.Himg, d.Wimg, d.rows_img, d.Cin, d.cstride, d.img_stride = H, hw // H, hw, K // 9 // 8 * 8, K // 9 // 8 * 8, hw * (K // 9 // 8 * 8)
            for g in groups:
                d.groups, d.gA, d.gW, d.gBias, d.gOut, d.gOut2 = g, 0, N * K, N, M * N, M * N
                for ws, nbytes in scratch:
                    d.splitk_ws = d.splitk_cnt = DUMMY if ws else None
                    d.splitk_ws_bytes = nbytes
                    for fl in flag_sets:
                        for k in flag_names:
                            setattr(d, k, fl.get(k, 0) or None if k in ("row_stats_in", "wsum", "row_stats_out", "row_stats_final", "row_stats_ticket", "max_out", "add") else fl.get(k, 0))
                        if epi != 2:
                            d.out2 = fl.get("out2")
                        for h in hints:
                            d.tile_hint = h
                            out.append(pick(ref) & 255)
        n += len(out)
        total.update(out)
        print("epi %d amode %d  %7d descriptors  picks %-44s sha256 %s" % (epi, amode, len(out), sorted(set(out)), hashlib.sha256(out).hexdigest()[:16]))
    print("all  %d descriptors  sha256 %s" % (n, total.hexdigest()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="regenerate tests/golden/gemm_pick_table.json")
    ap.add_argument("--sweep", action="store_true", help="digest of ud_gemm_pick over the wide product grid")
    ap.add_argument("--lib", help="another build of libunidepth_hip.so to ask (default: the tree's)")
    args = ap.parse_args()
    from unidepth_amd import _lib
    lib = _lib.lib
    if args.lib:
        lib = C.CDLL(args.lib)
        lib.ud_gemm_pick.argtypes = [C.POINTER(_lib.UdGemm)]
        assert lib.ud_struct_size(0) == C.sizeof(_lib.UdGemm)
    if args.sweep:
        sweep(lib)
        return 0
    table = build_table(lib)
    if args.write:
        write_table(table, GOLDEN)
        print("wrote %s: %d rows, %d labels" % (GOLDEN, sum(map(len, table.values())), len(table)))
        return 0
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {key(r): (p, l) for r, p, l in table_rows(table)}
    old = {key(r): (p, l) for r, p, l in table_rows(want)}
    bad = [(k, old.get(k), got.get(k)) for k in sorted(set(got) | set(old)) if old.get(k) != got.get(k)]
    for k, a, b in bad[:20]:
        print("golden %s, library %s: %s" % (a, b, k))
    print("%d rows, %d differ" % (len(got), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
