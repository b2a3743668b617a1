"""ctypes binding of csrc/libmi355rec.so, generated from the C ABI's own declaration, include/mi355rec.h.

The header is the one description of the boundary: this module reads it at import and derives the signature of every
entry point, the fields of ``DeepFMLazyAdam``, the ``REC_*`` defines (``LIMITS``: status codes and shape limits) and the
enumerators (``ENUMS``: operation codes) from it.  The type spellings it accepts are a closed set (the header's preamble
lists them); any other fails the import and names the declaration.

The HIP library is the product: there is NO fallback.  If the shared object is missing or a symbol the
header declares cannot be resolved, importing this module raises -- build it with
``python -c "import __graft_entry__ as g; g.build()"`` (or ``csrc/build.sh``).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmi355rec.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mi355rec.h")   # what csrc/build.sh compiles against

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
            "size_t": C.c_size_t}


class DeepFMLazyAdam(C.Structure):
    """rec_deepfm_lazy_adam of include/mi355rec.h: the optional lazy-Adam group of rec_deepfm_fused_post_f32 (its
    _fields_ are set from the header below)."""


def _ctype(decl, where, named=False):
    """'const float* const*' -> c_void_p, 'int64_t' -> c_int64, ...; with `named`, decl ends in the parameter's name.
    `where` names the declaration in the error."""
    words = decl.replace("*", " * ").split()
    stars = "*" in words
    words = [w for w in words if w not in ("const", "*")]
    base = words[0] if len(words) == 1 + named else None
    if stars and base == "rec_deepfm_lazy_adam":
        return C.POINTER(DeepFMLazyAdam)
    if stars and (base in _SCALARS or base == "void"):
        return C.c_void_p
    if not stars and base in _SCALARS:
        return _SCALARS[base]
    raise ImportError("include/mi355rec.h, %s: the bindings know no type like %r (the header's preamble lists the "
                      "spellings)" % (where, decl.strip()))


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def constants(text):
    """{name: value} of every `#define REC_<NAME> <integer>` (the value may stand in parentheses)."""
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(REC_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)
    return {name: int(value) for name, value in found}


def enums(text):
    """{name: value} of the enumerators of every `enum { A = 1, B, ... }`: an explicit integer, or one more than the
    enumerator before (0 for the first)."""
    out = {}
    for body in re.findall(r"\benum\s*\w*\s*\{([^{}]*)\}", text):
        nxt = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(\w+)(?:\s*=\s*\(?(-?\d+)\)?)?", item)
            if not m:
                raise ImportError("include/mi355rec.h: the bindings cannot read the enumerator %r" % item)
            nxt = int(m.group(2)) if m.group(2) is not None else nxt
            out[m.group(1)] = nxt
            nxt += 1
    return out


def struct_fields(text, struct):
    """ctypes _fields_ of `struct <struct> { ... }`: statements `type declarator, declarator;`, * on the declarator."""
    body = re.search(r"struct\s+%s\s*\{(.*?)\}" % struct, text, flags=re.S)
    if not body:
        raise ImportError("include/mi355rec.h does not define struct %s" % struct)
    fields = []
    for stmt in filter(None, (s.strip() for s in body.group(1).split(";"))):
        base, declarators = re.fullmatch(r"((?:const\s+)?\w+)\s*(.*)", stmt, flags=re.S).groups()
        for d in declarators.split(","):
            name = d.replace("*", "").strip()
            fields.append((name, _ctype(base + "*" * d.count("*"), "struct %s, field %s" % (struct, name))))
    return fields


def prototypes(text):
    """{symbol: (restype, argtypes)} of every prototype `ret rec_name(type name, ...);`."""
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    table = {}
    for ret, name, args in re.findall(r"(?:^|(?<=[;{}]))\s*([\w\s*]+?)\s*\b(rec_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [] if args.strip() == "void" else args.split(",")
        table[name] = (_ctype(ret, name), [_ctype(a, name, named=True) for a in args])
    return table


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(
            "%s not found: the ctypes bindings of the HIP extension are generated from it (the package is used from "
            "its source tree, next to include/)" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return strip_comments(f.read())


_header = _read_header()
LIMITS = constants(_header)                    # REC_OK, REC_E_*, REC_MAX_COLS and the kernel families' shape limits
ENUMS = enums(_header)                         # the operation codes REC_ACT_*, REC_EPI_*, REC_DACT_* that ops.py binds
DeepFMLazyAdam._fields_ = struct_fields(_header, "rec_deepfm_lazy_adam")
SIGNATURES = prototypes(_header)               # symbol -> (restype, argtypes), every function of include/mi355rec.h


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: the HIP extension is required (no CPU fallback exists). "
            "Build it with __graft_entry__.build() or csrc/build.sh" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # header / library out of sync
            raise ImportError("libmi355rec.so does not export %s: rebuild it" % name) from e
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()

# The hot operators are also registered with the PyTorch dispatcher -- TORCH_LIBRARY(mi355rec, ...) in csrc/torch_ops.cpp,
# a host-only wrapper over the SAME C ABI -- and ops.py calls them as torch.ops.mi355rec.<op>: one dispatcher hop per
# operator instead of a ctypes call with ~20 marshalled arguments.  Part of the product: missing -> ImportError.
TORCH_LIB_PATH = os.path.join(_HERE, "csrc", "libmi355rec_torch.so")


def _load_torch_ops():
    import torch
    if not os.path.exists(TORCH_LIB_PATH):
        raise ImportError("%s not found: build it with __graft_entry__.build() or csrc/build.sh" % TORCH_LIB_PATH)
    torch.ops.load_library(TORCH_LIB_PATH)
    return torch.ops.mi355rec


tops = _load_torch_ops()


class RecError(RuntimeError):
    pass


def check(status, what):
    if status == 0:
        return
    if status == -1:
        raise ValueError("%s: invalid argument" % what)
    if status == -2:
        raise NotImplementedError("%s: unsupported configuration" % what)
    if status == -3:
        raise RecError("%s: workspace too small" % what)
    raise RecError("%s: hipError_t %d" % (what, status))
