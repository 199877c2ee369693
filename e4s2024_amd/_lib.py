"""ctypes binding of ``libe4s_hip.so`` (the C ABI declared in ``include/e4s_hip.h``).

The library is built ahead of time (``python -m e4s2024_amd.build`` / ``__graft_entry__.build()``), never
at import.  There is no CPU fallback: if the shared object is missing or a symbol cannot be resolved the
import fails loudly, and every wrapper raises ``RuntimeError`` with the library's message on a non-zero status.

The header is the only description of the ABI: the prototypes, the two host structs and the ``E4S_*`` constants are read from it when this module is
imported, and the loaded library's ``e4s_abi_version()`` must be the header's.
"""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("E4S_HIP_LIB") or os.path.join(HERE, "lib", "libe4s_hip.so")   # E4S_HIP_LIB: tuning builds only
HEADER = os.path.join(os.path.dirname(HERE), "include", "e4s_hip.h")

c_int, c_i64, c_f32, c_ptr = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

# ---------------------------------------------------------------------------- the header is the one description of the ABI
_SCALARS = {"int": c_int, "int64_t": c_i64, "float": c_f32, "unsigned": ctypes.c_uint}
_RETURNS = {"int": c_int, "const char*": ctypes.c_char_p}


def _ctype(decl: str, where: str):
    """The ctypes type of one C declaration ``<type> <name>``: any pointer is ``void*``, a scalar goes by its type's name, anything else is refused."""
    if "*" in decl:
        return c_ptr
    ty = " ".join(decl.split()[:-1])
    if ty not in _SCALARS:
        raise TypeError(f"{where}: no ctypes rule for '{' '.join(decl.split())}' (known: pointers, {', '.join(_SCALARS)})")
    return _SCALARS[ty]


def parse_header(text: str):
    """``(protos, restypes, structs, defines)`` of the ABI header's text: ``{entry point: [argument ctypes]}``, ``{entry point: return ctype}``,
    ``{struct: [(field, ctype)]}`` in declaration order and ``{E4S_NAME: int}``.  Not a C parser: it knows the forms include/e4s_hip.h uses
    (``E4S_API <ret> e4s_name(<type> <name>, ...);``, ``typedef struct Name { <type> <name>[, <name>]; ... }``, ``#define E4S_NAME <int>``) and
    raises ``TypeError``, naming the place, on a type it has no rule for."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(E4S_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", code, flags=re.M)}
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^}]*)\}", code):
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            ty = _ctype(first, f"struct {name}")
            if more and ty is c_ptr:
                raise TypeError(f"struct {name}: no ctypes rule for a list of pointers, '{decl}'")
            fields += [(n.split()[-1].strip("*"), ty) for n in [first] + more]
    protos, restypes = {}, {}
    for ret, name, args in re.findall(r"E4S_API\s+([\w\s*]+?)\s*\b(e4s_\w+)\s*\(([^()]*)\)\s*;", code):
        ret = " ".join(ret.split())
        if ret not in _RETURNS:
            raise TypeError(f"{name}: no ctypes rule for the return type '{ret}' (known: {', '.join(_RETURNS)})")
        restypes[name] = _RETURNS[ret]
        args = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = [_ctype(a, f"{name}: argument {i}") for i, a in enumerate(args)]
    if len(protos) != len(re.findall(r"\bE4S_API\b", code)):
        raise TypeError(f"the header has {len(re.findall('E4S_API', code))} E4S_API declarations, {len(protos)} were understood")
    return protos, restypes, structs, defines


with open(HEADER) as _f:
    _PROTOS, _RESTYPES, _STRUCTS, _DEFINES = parse_header(_f.read())          # name -> argtypes, for every entry point

ABI_VERSION, ERR_ARG, MAX_REGIONS, LABEL_NONE, MAX_STYLE_JOBS, MAX_TARGETS, X_NHWC, OUT_NHWC, X_SP, OUT_SP = (_DEFINES["E4S_" + n] for n in (
    "ABI_VERSION", "ERR_ARG", "MAX_REGIONS", "LABEL_NONE", "MAX_STYLE_JOBS", "MAX_TARGETS", "X_NHWC", "OUT_NHWC", "X_SP", "OUT_SP"))


def targets(ptrs, weights):
    """The ``(ys, tw, k)`` arguments of the multi-target entry points: host arrays of the targets' device pointers and of their weights."""
    k = len(ptrs)
    if not 1 <= k <= MAX_TARGETS or len(weights) != k:
        raise ValueError(f"1 .. {MAX_TARGETS} targets with one weight each, got {k} targets and {len(weights)} weights")
    return (c_ptr * k)(*ptrs), (c_f32 * k)(*[float(w) for w in weights]), k


def declared_symbols():
    """Names of every entry point declared in include/e4s_hip.h."""
    return list(_PROTOS)


class StyleJob(ctypes.Structure):
    """E4sStyleJob (include/e4s_hip.h)."""
    _fields_ = _STRUCTS["E4sStyleJob"]


class ChainLayer(ctypes.Structure):
    """E4sChainLayer (include/e4s_hip.h)."""
    _fields_ = _STRUCTS["E4sChainLayer"]


class _Lib:
    def __init__(self):
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} not found: build the HIP library first (python -m e4s2024_amd.build). "
                "e4s2024_amd has no CPU fallback.")
        # torch first: its wheel carries its own libamdhip64, and the process must end up with ONE HIP runtime — the library loaded before torch
        # brings in /opt/rocm's copy, torch then its own, and the kernels launch into a runtime that has no device ("no ROCm-capable device")
        import torch  # noqa: F401
        self.cdll = ctypes.CDLL(SO_PATH)
        if self.cdll.e4s_abi_version() != ABI_VERSION:
            raise ImportError(f"{SO_PATH} has ABI version {self.cdll.e4s_abi_version()}, include/e4s_hip.h declares {ABI_VERSION}: rebuild it "
                              "(python -m e4s2024_amd.build)")
        self._entry = {}                   # name -> (function, argument count)
        for name, args in _PROTOS.items():
            fn = getattr(self.cdll, name)  # AttributeError if the .so is stale
            fn.argtypes = args
            fn.restype = _RESTYPES[name]
            self._entry[name] = (fn, len(args))
        self.path = SO_PATH

    def call(self, name: str, *args):
        fn, nargs = self._entry[name]
        if len(args) != nargs:             # ctypes itself accepts extra arguments to a cdecl function
            raise TypeError(f"{name} takes {nargs} arguments, {len(args)} given")
        st = fn(*args)
        if st != 0:
            raise RuntimeError(f"{name} failed (status {st}): {self.cdll.e4s_last_error().decode()}")


_lib = None


def lib() -> _Lib:
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
