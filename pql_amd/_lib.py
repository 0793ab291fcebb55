"""ctypes binding of libpqlk.so, derived from include/pqlk.h: the header is the only declaration of the C ABI.

The library is the product: if it is missing or fails to load this module raises, there is no
CPU or eager-PyTorch fallback anywhere in pql_amd.

`parse_header` reads the header once at import.  It accepts, and must consume to the last character, this grammar:
  /* ... */                               dropped first, so a declaration may carry comments anywhere
  #ifndef X / #define X (the guard pair), #ifdef, #endif, #include lines; extern "C" { ... }      dropped
  #define PQLK_NAME <integer>             constant NAME (module attribute `NAME`: ACT_TANH, GATHER_CLAMP5, VERSION, ...)
  #define PQLK_NAME(args) ...             a function-like macro: skipped
  enum { PQLK_A = <integer>, ... };       constants; every value is explicit
  typedef void* name;                     `name` is c_void_p (pqlk_stream_t)
  typedef struct [Tag] { type field; type field[expr]; ... } Name;
                                          ctypes.Structure `Name` (module attribute; fields in order); expr is integer arithmetic
                                          over the constants; a pointer field is c_void_p
  ret pqlk_name(type arg, ...);           PROTOTYPES[pqlk_name] = (restype, [argtypes]), in header order; may span lines; `(void)`
Types: int, int32_t, int64_t, uint32_t, uint64_t, float, double -> the ctypes class of that name; a `typedef void*` name ->
c_void_p; `const char*` as a return -> c_char_p; [const] Struct* -> POINTER(Struct); [const] T* for T one of those scalars, void,
uint8_t or uint16_t -> c_void_p (device pointers, and host out-pointers given as byref() or a ctypes array).  Anything else --
size_t, long, a struct the header does not define, text between declarations -- is an ImportError that quotes it.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

import torch

_HERE = Path(__file__).resolve().parent
LIB_FILE = Path(os.environ.get("PQLK_LIB", _HERE / "csrc" / "libpqlk.so"))   # PQLK_LIB: A/B a tuning build
HEADER_FILE = _HERE.parent / "include" / "pqlk.h"   # the file csrc/pqlk_common.h includes

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = {*_SCALARS, "void", "uint8_t", "uint16_t"}
_TYPE = r"(?P<const>const\s+)?(?P<base>\w+)(?P<ptr>\s*\*\s*|\s+)"   # `[const] base` then `*` or the space before the name
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"


def parse_header(text: str, where="header"):
    """-> (constants {NAME: int}, structs {Name: Structure class}, prototypes {pqlk_name: (restype, [argtypes])})."""
    consts, structs, aliases, protos = {}, {}, {}, {}

    def fail(what, decl):
        raise ImportError(f"{where}: {what}: {' '.join(decl.split())!r}")

    def ctype(m, decl, ret=False, field=False):
        base, ptr = m["base"], "*" in m["ptr"]
        if not ptr and base in _SCALARS:
            return _SCALARS[base]
        if not ptr and base in aliases:
            return aliases[base]
        if not ptr and ret and base == "void":
            return None
        if ptr and ret and base == "char" and m["const"]:
            return C.c_char_p
        if ptr and base in structs and not field:
            return C.POINTER(structs[base])
        if ptr and base in _POINTEES:
            return C.c_void_p
        fail(f"type {(m['const'] or '') + base + ('*' if ptr else '')!r} is not in the type law", decl)

    def define(m):
        consts[m[1]] = int(m[2], 0)

    def enum(m):
        for item in filter(None, (s.strip() for s in m[1].split(","))):
            e = re.fullmatch(rf"PQLK_(\w+)\s*=\s*({_INT})", item) or fail("an enumerator needs an explicit integer value", m[0])
            consts[e[1]] = int(e[2], 0)

    def struct(m):
        fields = []
        for item in filter(None, (s.strip() for s in m[1].split(";"))):
            f = re.fullmatch(_TYPE + r"(?P<name>\w+)\s*(?:\[(?P<n>[^\]]*)\])?", item) or fail("not a `type name;` field", item)
            t = ctype(f, m[0], field=True)
            if f["n"] is not None:
                expr = re.sub(r"PQLK_(\w+)", lambda c: str(consts[c[1]]) if c[1] in consts else fail("unknown constant", item), f["n"])
                re.fullmatch(r"[\d\s+*()-]+", expr) or fail("an array size is integer arithmetic over the constants", item)
                t = t * int(eval(expr, {"__builtins__": {}}))
            fields.append((f["name"], t))
        structs[m[2]] = type(m[2], (C.Structure,), {"_fields_": fields})

    def alias(m):
        aliases[m[1]] = C.c_void_p

    def function(m):
        args = [] if m["args"].strip() == "void" else m["args"].split(",")
        parsed = [re.fullmatch(_TYPE + r"\w+", a.strip()) or fail("not a `type name` argument", m[0]) for a in args]
        protos[m["name"]] = (ctype(m, m[0], ret=True), [ctype(a, m[0]) for a in parsed])

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#ifndef\s+(\w+)\s*\n[ \t]*#define\s+\1[ \t]*$", "", text, flags=re.M)
    text = re.sub(r"^[ \t]*#(?:ifndef|ifdef|endif|include)\b.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    for pattern, action in ((r"^[ \t]*#define\s+PQLK_\w+\(.*$", lambda m: None),
                            (rf"^[ \t]*#define\s+PQLK_(\w+)[ \t]+({_INT})[ \t]*$", define),
                            (r"\benum\s*\{([^{}]*)\}\s*;", enum),
                            (r"\btypedef\s+void\s*\*\s*(\w+)\s*;", alias),
                            (r"\btypedef\s+struct\s*(?:\w+\s*)?\{([^{}]*)\}\s*(\w+)\s*;", struct),
                            (_TYPE + r"(?P<name>pqlk_\w+)\s*\((?P<args>[^()]*)\)\s*;", function)):
        text = re.sub(pattern, lambda m: action(m) or "", text, flags=re.M)
    if text.strip():
        fail("text that is no declaration the binding understands", text.strip()[:120])
    return consts, structs, protos


def load_header(path=HEADER_FILE):
    try:
        text = Path(path).read_text()
    except OSError as e:
        raise ImportError(f"{path} is missing or unreadable ({e.strerror}): the ctypes binding is derived from it") from e
    return parse_header(text, where=os.fspath(path))


CONSTANTS, STRUCTS, PROTOTYPES = load_header()   # PROTOTYPES: name -> (restype, argtypes), in the header's order
globals().update(CONSTANTS)   # PQLK_X -> X: MAX_LAYERS, OBS_*, INFO_*, ACT_*, GATHER_*, STASH_OUTPUT_ONLY, E_*, VERSION, ...
globals().update(STRUCTS)     # PqlReplayDesc, PqlMlpDesc, PqlInfoKey


def _load():
    if not LIB_FILE.exists():
        raise ImportError(
            f"{LIB_FILE} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {LIB_FILE.parent}`. pql_amd has no fallback path.")
    lib = C.CDLL(os.fspath(LIB_FILE))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()


class PqlkError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        raise PqlkError(f"{lib.pqlk_strerror(rc).decode()} (rc={rc})")


def ld(cols: int) -> int:
    return int(lib.pqlk_ld(int(cols)))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device=None):
    """hipStream_t of torch's current stream: kernels run in order with torch ops and can be graph-captured."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(t: torch.Tensor, name="tensor"):
    if not t.is_cuda:
        raise PqlkError(f"{name} must live on an MI355X device (got {t.device}); pql_amd has no CPU path")
    if t.dtype not in (torch.float32, torch.int64, torch.int32):
        raise PqlkError(f"{name}: unsupported dtype {t.dtype}")
    if not t.is_contiguous():
        raise PqlkError(f"{name} must be contiguous")
    return t


def mlp_desc(dims, n_nets=1) -> PqlMlpDesc:
    dims = [int(x) for x in dims]
    if not (2 <= len(dims) <= MAX_LAYERS + 1):
        raise PqlkError("MLP needs between 1 and 8 Linear layers")
    d = PqlMlpDesc()
    d.n_layers, d.n_nets = len(dims) - 1, int(n_nets)
    for i, x in enumerate(dims):
        d.dims[i] = x
    return d
