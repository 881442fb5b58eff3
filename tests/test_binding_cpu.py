"""The whole ctypes binding (unidepth_amd/_lib.py) against include/unidepth_hip.h, parsed once by tests/header_decl.py: every descriptor
struct field by field, every index of ud_struct_size, every function's argument and return types, every UD_* constant, and the version.
Needs only the built library, no GPU."""
import ctypes as C
import os
import re

import pytest

import header_decl as hd
from unidepth_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS, PROTOTYPES, CONSTANTS = hd.structs(_lib), hd.prototypes(_lib), hd.constants()
INDEX, UNASSIGNED = hd.struct_indices(), hd.unassigned_indices()
MIRRORS = {n: v for n, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, C.Structure)}
BOUND_CONSTANTS = {n: v for n, v in vars(_lib).items() if n.startswith("UD_") and isinstance(v, int)}
RAW_LIB = C.CDLL(_lib.LIB_PATH)


def _differences(got, want):
    """positions at which two lists of ctypes types (None: no type at all) differ"""
    if got is None or len(got) != len(want):
        return [("length", got and len(got), len(want))]
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if not hd.same_type(g, w)]


# ---- structs -------------------------------------------------------------------------------------------------------------------------

def test_the_parser_sees_the_whole_header():
    assert len(STRUCTS) == len(re.findall(r"\btypedef\s+struct\s+\w+\s*\{", hd.SRC)) >= 41
    assert len(PROTOTYPES) == len(set(re.findall(r"\b(ud_\w+)\s*\(", hd.SRC))) >= 101
    assert len(CONSTANTS) == len(set(re.findall(r"#\s*define\s+(UD_\w+)", hd.SRC)) | set(re.findall(r"\b(UD_\w+)\s*=", hd.SRC)))


@pytest.mark.parametrize("name", list(STRUCTS))
def test_struct_mirror_equals_the_header(name):
    mirror = MIRRORS.get(name)
    assert mirror is not None, f"_lib has no ctypes.Structure named {name}"
    want, got = STRUCTS[name], list(mirror._fields_)
    assert [f for f, _ in got] == [f for f, _ in want], f"{name}: field names or their order differ from the header"
    bad = [(want[i][0], g, w) for i, g, w in _differences([t for _, t in got], [t for _, t in want])]
    assert not bad, f"{name}: (field, binding's type, header's type) {bad}"


def test_every_mirror_has_a_header_struct():
    assert set(MIRRORS) == set(STRUCTS)


# ---- ud_struct_size ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(INDEX))
def test_struct_size_at_its_index(name):
    i = INDEX[name]
    assert _lib.STRUCT_INDEX.get(i) is MIRRORS[name], f"{name}: the header gives index {i}, _lib.STRUCT_INDEX holds {_lib.STRUCT_INDEX.get(i)}"
    assert _lib.lib.ud_struct_size(i) == C.sizeof(MIRRORS[name]), name


def test_index_tables_agree_and_unassigned_numbers_answer_minus_one():
    assert {i: st.__name__ for i, st in _lib.STRUCT_INDEX.items()} == {i: n for n, i in INDEX.items()}
    assert len(set(INDEX.values())) == len(INDEX)
    top = max(INDEX.values())
    assert sorted(UNASSIGNED) == sorted(set(range(top + 1)) - set(INDEX.values()))          # exactly the gaps
    for i in UNASSIGNED + [-1, top + 1]:
        assert _lib.lib.ud_struct_size(i) == -1, i


def test_every_struct_is_covered_by_a_size_check():
    """a struct without an index of its own is a member of an indexed one, so the import-time size check covers its layout too"""
    covered = {MIRRORS[n] for n in INDEX}
    grew = True
    while grew:
        inner = {getattr(t, "_type_", t) if issubclass(t, C.Array) else t for st in covered for _, t in st._fields_}
        inner = {t for t in inner if issubclass(t, C.Structure)} - covered
        covered |= inner
        grew = bool(inner)
    assert sorted(set(STRUCTS) - {st.__name__ for st in covered}) == []            # no exception so far; name any here, with its reason


# ---- functions -----------------------------------------------------------------------------------------------------------------------

def test_the_binding_binds_exactly_the_declared_functions():
    assert set(_lib.SIG) == set(PROTOTYPES)
    assert set(_lib.RESTYPE) <= set(_lib.SIG)


@pytest.mark.parametrize("name", list(PROTOTYPES))
def test_prototype_equals_the_header(name):
    restype, argtypes = PROTOTYPES[name]
    assert hasattr(RAW_LIB, name), f"the library does not export {name}"
    fn = getattr(_lib.lib, name)
    assert fn.restype is restype, f"{name}: returns {restype} by the header, {fn.restype} in the binding"
    bad = _differences(fn.argtypes, argtypes)
    assert not bad, f"{name}: (argument, binding's type, header's type) {bad}"


# ---- constants and version -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BOUND_CONSTANTS))
def test_constant_equals_the_header(name):
    assert name in CONSTANTS, f"{name} is not a constant of the header"
    assert BOUND_CONSTANTS[name] == CONSTANTS[name], name


def test_header_constants_the_binding_does_not_name():
    """a listing, not a requirement: not every constant is needed from Python"""
    missing = sorted(set(CONSTANTS) - set(BOUND_CONSTANTS))
    print("header constants without a name in _lib:", ", ".join(missing))
    assert set(missing) <= set(CONSTANTS), missing


def test_version_is_the_one_the_library_source_states():
    with open(os.path.join(ROOT, "unidepth_amd", "csrc", "api.cpp")) as f:
        literal = re.search(r"\bud_version\s*\(\s*void\s*\)\s*\{\s*return\s+(\d+)\s*;", f.read()).group(1)
    assert _lib.lib.ud_version() == int(literal)
