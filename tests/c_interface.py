"""The C interface as the headers under include/ state it, for the tests: a declaration parser (functions, structs, integer constants
mapped to ctypes), the error codes read from the header's enum, host memory standing in for device pointers, and ``entry`` - a caller
of one entry point by the header's own parameter names, for the refusal tests."""
import ctypes as C
import keyword
import os
import re

from lkgd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")

_STRUCT_PTR = {"lkgd_gemm_desc": C.POINTER(_lib.GemmDesc), "lkgd_gemm_plan_info": C.POINTER(_lib.GemmPlanInfo),
               "lkgd_fsm_desc": C.POINTER(_lib.FsmDesc)}
_SCALAR = {"int32_t": C.c_int32, "int": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "lkgd_stream_t": C.c_void_p}
_RETURN = {"int": C.c_int32, "void": None, "const char*": C.c_char_p}


def _text(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def _ctype(ctype):
    """the ctypes type of a C parameter or field type: any pointer is a void pointer, but for the three described structures"""
    words = ctype.replace("*", " * ").split()
    if "*" in words:
        return next((_STRUCT_PTR[w] for w in words if w in _STRUCT_PTR), C.c_void_p)
    (word,) = [w for w in words if w != "const"]
    return _SCALAR[word]


def functions(header):
    """{name: (restype, [(parameter name, ctype), ...])} of every ``<ret> lkgd_name(<params>);`` of the header, in its order"""
    out = {}
    for ret, name, params in re.findall(r"^(int|void|const char\*) (lkgd_[a-z0-9_]+)\s*\(([^)]*)\);", _text(header), re.M):
        assert name not in out, name
        rows = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            ctype, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, re.S).groups()
            rows.append((pname, _ctype(ctype)))
        out[name] = (_RETURN[ret], rows)
    return out


def structs(header):
    """{name: [(field, ctype), ...]} of every ``typedef struct name { ... } name;`` (``int32_t M, N, K;`` declares three fields)"""
    out = {}
    for name, body, name2 in re.findall(r"typedef struct (\w+) \{(.*?)\}\s*(\w+);", _text(header), re.S):
        assert name == name2, (name, name2)
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            first, *more = stmt.split(",")
            ctype, fname = re.fullmatch(r"(.*?)(\w+)", first.strip(), re.S).groups()
            fields += [(f.strip(), _ctype(ctype)) for f in [fname] + more]
        out[name] = fields
    return out


def constants(header):
    """{NAME: int} of every enumerator ``LKGD_NAME = <integer>`` of the header's enums"""
    out = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", _text(header), re.S):
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, value = re.fullmatch(r"(LKGD_\w+)\s*=\s*(-?\d+)", item).groups()     # anything else is an error, not a gap
            assert name not in out, name
            out[name] = int(value)
    return out


#: every function of every header of ``_lib.HEADERS``: name -> (restype, [(parameter name, ctype), ...])
FUNCTIONS = {name: sig for header in _lib.HEADERS for name, sig in functions(header).items()}

_codes = constants("lkgd_hip.h")
OK, NULL, SHAPE, ALIGN, MODE, LAUNCH = (_codes[k] for k in ("LKGD_OK", "LKGD_E_NULL", "LKGD_E_SHAPE", "LKGD_E_ALIGN", "LKGD_E_MODE",
                                                             "LKGD_E_LAUNCH"))


class Host:
    """host memory standing in for device pointers: a refused call never launches, so nothing dereferences them (only the
    array `w` is read on the host)"""

    def __init__(self):
        self.buf = C.create_string_buffer(4096 + 64)
        base = C.addressof(self.buf)
        self.p = (base + 63) & ~63           # 64-byte aligned
        self.w = (C.c_void_p * 18)(*[self.p] * 18)


def entry(name, **defaults):
    """a caller of the entry point ``name``: ``defaults`` names exactly the header's parameters (a trailing ``stream`` may be left out
    and is then NULL); ``call(**overrides)`` passes them in the header's order and returns the code.  A key that is no parameter of
    the header's declaration is an error, in the defaults and in every call.  A parameter whose C name is a Python keyword takes a
    trailing underscore (``in_``)."""
    order = [p + "_" * keyword.iskeyword(p) for p, _ in FUNCTIONS[name][1]]
    if order and order[-1] == "stream":
        defaults.setdefault("stream", None)
    if set(defaults) != set(order):
        raise TypeError(f"{name}: defaults lack {sorted(set(order) - set(defaults))}, unknown {sorted(set(defaults) - set(order))}")
    fn = getattr(_lib.lib(), name)

    def call(**overrides):
        if not set(overrides) <= set(order):
            raise TypeError(f"{name}: no parameter named {sorted(set(overrides) - set(order))}")
        args = {**defaults, **overrides}
        return fn(*[args[p] for p in order])
    return call
