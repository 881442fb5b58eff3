"""The one parser of include/unidepth_hip.h for the tests (a helper, not a test module): its constants, descriptor structs, function
prototypes and the struct-index table of ud_struct_size, each in the ctypes terms of unidepth_amd/_lib.py, so that
tests/test_binding_cpu.py can compare the whole binding with the header."""
import ctypes as C
import keyword
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidepth_hip.h")
with open(HEADER) as _f:
    RAW = _f.read()
SRC = re.sub(r"/\*.*?\*/|//[^\n]*", " ", RAW, flags=re.S)                      # no comments

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long long": C.c_longlong, "float": C.c_float,
           "double": C.c_double, "unsigned char": C.c_ubyte, "size_t": C.c_size_t}
_RETURNS = {"void": None, "char*": C.c_char_p, "UdProgram*": C.c_void_p}


def constants():
    """{name: int} of every `#define UD_X <int>` (parenthesised, negative and hex values too) and every `enum { UD_X = n, ... }`."""
    out = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(UD_\w+)[ \t]+\(?[ \t]*(%s)[ \t]*\)?[ \t]*$" % _INT, SRC, re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}", SRC, re.S):
        out.update({n: int(v, 0) for n, v in re.findall(r"\b(UD_\w+)\s*=\s*(%s)" % _INT, body)})
    return out


def _words(text):
    return " ".join(re.sub(r"\bconst\b", " ", text).split())


def structs(lib_module):
    """Ordered {struct name: [(field, ctype), ...]} of every `typedef struct X { ... } X;`.  Pointers of any kind are c_void_p, an earlier
    struct is its mirror in lib_module, name[N] is ctype * N (N a literal or a constant), a Python keyword gets a trailing underscore."""
    consts, out = constants(), {}
    for name, body in _STRUCT.findall(SRC):
        fields = []
        for decl in filter(None, (_words(d) for d in body.split(";"))):
            first, *more = decl.split(",")
            m = re.match(r"(.*?)([\s*]+)(\w+)\s*(?:\[(\w+)\])?$", first)            # base type, stars, name, [length]
            assert m, (name, decl)
            base = m.group(1).strip()
            declarators = [m.groups()[1:]] + [re.match(r"([\s*]*)(\w+)\s*(?:\[(\w+)\])?$", d).groups() for d in more]
            for stars, field, length in declarators:
                assert "*" in stars or base in SCALARS or base in out, (name, decl)
                ct = C.c_void_p if "*" in stars else SCALARS[base] if base in SCALARS else getattr(lib_module, base)
                if length is not None:
                    ct = ct * (int(length) if length.isdigit() else consts[length])
                fields.append((field + "_" if keyword.iskeyword(field) else field, ct))
        out[name] = fields
    return out


def prototypes(lib_module):
    """{function name: (restype, [argtypes])} of every ud_* declaration, by the binding's conventions: a pointer to a descriptor struct is
    POINTER(mirror), char* is c_char_p, double* is POINTER(c_double), every other pointer (UdProgram* too) is c_void_p."""
    names = [n for n, _ in _STRUCT.findall(SRC)]
    text = re.sub(r"^[ \t]*#.*$", " ", _STRUCT.sub(" ", SRC), flags=re.M).replace('extern "C" {', " ")
    out = {}
    for stmt in text.split(";"):
        m = re.match(r"\s*([\w\s*]+?)\s*\b(ud_\w+)\s*\((.*)\)\s*$", stmt, re.S)
        if not m:
            continue
        ret, fn, params = _words(m.group(1)), m.group(2), _words(m.group(3))
        args = []
        for p in ([] if params in ("", "void") else params.split(",")):
            if "*" in p:
                base = p.split("*")[0].strip()
                args.append(C.POINTER(getattr(lib_module, base)) if base in names else C.c_char_p if base == "char"
                            else C.POINTER(C.c_double) if base == "double" else C.c_void_p)
            else:
                p = p.strip()
                args.append(SCALARS[p] if p in SCALARS else SCALARS[p.rsplit(" ", 1)[0]])        # unnamed, or the type without the name
        ret = re.sub(r"\s*\*", "*", ret)
        restype = _RETURNS[ret] if ret in _RETURNS else SCALARS[ret]
        assert fn not in out, fn
        out[fn] = (restype, args)
    return out


def _index_comment():
    return re.search(r"/\*(?:(?!\*/).)*?ud_struct_size\(i\)(.*?)\*/", RAW, re.S).group(1)


def struct_indices():
    """{struct name: index} as the comment above ud_struct_size lists them."""
    return {n: int(i) for n, i in re.findall(r"\b(Ud\w+) = (\d+)", _index_comment())}


def unassigned_indices():
    """the numbers that the same comment says are not assigned"""
    return [int(i) for i in re.findall(r"\d+", re.search(r";([^;]*?)are not assigned", _index_comment(), re.S).group(1))]


def same_type(a, b):
    """ctypes types compared by value: arrays by element type and length, pointers by target."""
    if isinstance(a, type) and isinstance(b, type) and issubclass(a, C.Array) and issubclass(b, C.Array):
        return a._length_ == b._length_ and same_type(a._type_, b._type_)
    if isinstance(a, type) and isinstance(b, type) and issubclass(a, C._Pointer) and issubclass(b, C._Pointer):
        return same_type(a._type_, b._type_)
    return a is b
