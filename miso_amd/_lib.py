"""ctypes binding of libmiso_hip.so (C ABI in include/miso_hip.h).

The library is the product: there is no CPU or PyTorch fallback for the hot ops.
A missing library, or a call with tensors that are not on a HIP device, raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

# torch must be imported BEFORE libmiso_hip.so is loaded: both need
# libamdhip64.so.7 and the process must end up with the ONE HIP runtime torch
# ships (loading ROCm's copy first leaves torch without a device).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MISO_HIP_LIB: a dev override for A/B runs of differently built libraries, tools/train_ab.sh)
LIB_PATH = os.environ.get("MISO_HIP_LIB") or os.path.join(_HERE, "libmiso_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "miso_hip.h")
HASH_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "miso_hash.h")     # hash-indexed levels: tables of its own
HASH_SDF_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "miso_hash_sdf.h")     # their fused SDF query: likewise
HASH_TRACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "miso_hash_trace.h")     # sphere tracing through them


class HeaderError(RuntimeError):
    """include/miso_hip.h holds something the reader below does not understand."""


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint8_t": C.c_uint8,
            "int8_t": C.c_int8, "float": C.c_float, "double": C.c_double}
# Pointers are c_void_p (callers pass tensor.data_ptr(), None or a small host array) except where a caller hands over a
# typed ctypes pointer, which a c_void_p FIELD refuses: ops.RaySampler stores cast(edges, POINTER(c_float)).
_TYPED_POINTERS = {"miso_ray_sampling_t.bin_edges": C.POINTER(C.c_float)}


def _ctype(spec, structs, where):
    """'const float*', 'int64_t', 'miso_grid_t', 'const miso_mlp_t*' ... -> the ctypes type"""
    words = [w for w in spec.replace("*", " * ").split() if w != "const"]
    if len(words) == 1 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    if len(words) == 1 and words[0] in structs:
        return structs[words[0]]
    if len(words) == 2 and words[1] == "*":
        if words[0] in structs:
            return C.POINTER(structs[words[0]])
        if words[0] == "char":
            return C.c_char_p
        if words[0] == "void" or words[0] in _SCALARS:
            return _TYPED_POINTERS.get(where, C.c_void_p)
    raise HeaderError(f"{where}: unknown type '{spec.strip()}'")


def _declarator(text, where):
    """'const float* weight[MISO_MAX_LINEAR]' -> ('const float*', 'weight', 'MISO_MAX_LINEAR' or None)"""
    m = re.fullmatch(r"(?:(.*[\s*]))?(\w+)\s*(?:\[\s*(\w+)\s*\])?", text.strip())
    if not m:
        raise HeaderError(f"{where}: cannot split '{text.strip()}'")
    return (m[1] or "").strip(), m[2], m[3]


def read_header(text, base=None):
    """The C ABI as miso_hip.h declares it: (constants, structs, signatures), keyed by the C names.  The header is
    plain C in a narrow style (see its declarations); anything outside that style raises HeaderError, never skips.
    base: (constants, structs) of the header this one includes -- its declarations may use them; what comes back is
    this header's own."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts, structs, sigs, code, cpp_only = {}, {}, {}, [], False
    known_consts, known_structs = (dict(base[0]), dict(base[1])) if base else ({}, {})
    for line in text.split("\n"):
        d = line.split()
        if not d or not d[0].startswith("#"):
            if not cpp_only:
                code.append(line)
            elif d not in ([], ["extern", '"C"', "{"], ["}"]):            # the C++ wrapper and nothing else
                raise HeaderError(f"cannot read '{line.strip()}'")
        elif d[0] == "#define":
            m = re.fullmatch(r"#define (MISO_\w+) (\d+)u?", " ".join(d))
            if m:
                consts[m[1]] = int(m[2])
            elif d[1:] not in (["MISO_HIP_H"], ["MISO_HASH_H"], ["MISO_HASH_SDF_H"], ["MISO_HASH_TRACE_H"]) and not d[1].startswith("MISO_TILES_XYZ("):  # guards; ops.pack_tiles
                raise HeaderError(f"cannot read '{line.strip()}'")
        elif d[:2] == ["#ifdef", "__cplusplus"] or d[0] == "#endif":
            cpp_only = d[0] == "#ifdef"
        elif d[0] not in ("#include", "#ifndef"):
            raise HeaderError(f"cannot read '{line.strip()}'")

    def count(n, where):
        if not n.isdigit() and n not in consts and n not in known_consts:
            raise HeaderError(f"{where}: unknown array size '{n}'")
        return int(consts.get(n, known_consts.get(n, n)))

    def struct(m):
        name, fields = m[2], []
        for decl in filter(str.strip, m[1].split(";")):
            for i, piece in enumerate(decl.split(",")):          # int32_t C, Z, Y, X;  float bound_min[3], bound_max[3];
                s, field, n = _declarator(piece, name)
                spec = s if i == 0 else spec
                if bool(s) != (i == 0) or (i and "*" in spec):   # in C a '*' belongs to one declarator, not to the list
                    raise HeaderError(f"{name}: cannot split '{decl.strip()}'")
                t = _ctype(spec, {**known_structs, **structs}, f"{name}.{field}")
                fields.append((field, t if n is None else t * count(n, name)))
        camel = "".join(w.capitalize() for w in name[len("miso_"):-len("_t")].split("_"))
        structs[name] = type(camel, (C.Structure,), {"_fields_": fields})
        return " "

    code = re.sub(r"typedef\s+struct\s*\{([^{}]*)\}\s*(miso_\w+_t)\s*;", struct, "\n".join(code))
    for proto in filter(str.strip, code.split(";")):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(miso_\w+)\s*\(([^()]*)\)\s*", proto)
        if not m:
            raise HeaderError(f"cannot read '{proto.strip()[:80]}'")
        args = [] if m[3].strip() == "void" else [_declarator(a, m[2]) for a in m[3].split(",")]
        if any(n is not None or not spec for spec, _, n in args):
            raise HeaderError(f"{m[2]}: cannot read '{m[3].strip()}'")
        every = {**known_structs, **structs}
        sigs[m[2]] = (_ctype(m[1], every, m[2]), [_ctype(spec, every, f"{m[2]}({arg})") for spec, arg, _ in args])
    return consts, structs, sigs


with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, SIGNATURES = read_header(_f.read())   # SIGNATURES: name -> (restype, argtypes)
# the names the package uses: MISO_F_CROWDED -> F_CROWDED, MISO_MAX_LEVELS -> MAX_LEVELS, miso_lm_track_t -> LmTrack ...
globals().update({k[len("MISO_"):]: v for k, v in CONSTANTS.items()})
globals().update({s.__name__: s for s in STRUCTS.values()})
# include/miso_hash.h, read the same way into tables of its own: SIGNATURES / STRUCTS describe miso_hip.h alone
with open(HASH_HEADER_PATH) as _f:
    HASH_CONSTANTS, HASH_STRUCTS, HASH_SIGNATURES = read_header(_f.read(), base=(CONSTANTS, STRUCTS))
globals().update({k[len("MISO_"):]: v for k, v in HASH_CONSTANTS.items()})      # HASH_LOG2_MIN, HASH_LOG2_MAX
globals().update({s.__name__: s for s in HASH_STRUCTS.values()})                # HashLevel, HashGrid
# include/miso_hash_sdf.h: function declarations over the types of the two headers above, again in tables of its own
with open(HASH_SDF_HEADER_PATH) as _f:
    HASH_SDF_CONSTANTS, HASH_SDF_STRUCTS, HASH_SDF_SIGNATURES = read_header(
        _f.read(), base=({**CONSTANTS, **HASH_CONSTANTS}, {**STRUCTS, **HASH_STRUCTS}))
# include/miso_hash_trace.h: likewise
with open(HASH_TRACE_HEADER_PATH) as _f:
    HASH_TRACE_CONSTANTS, HASH_TRACE_STRUCTS, HASH_TRACE_SIGNATURES = read_header(
        _f.read(), base=({**CONSTANTS, **HASH_CONSTANTS}, {**STRUCTS, **HASH_STRUCTS}))

_lib = None


def load():
    """Load libmiso_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C miso_amd/csrc`.  miso_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **HASH_SIGNATURES, **HASH_SDF_SIGNATURES, **HASH_TRACE_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError = ABI mismatch, fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class MisoError(RuntimeError):
    """A call of the library came back with ``code`` (a MISO_E_* value or a hipError_t); ``what``: the entry's name."""

    def __init__(self, message, code, what):
        super().__init__(message)
        self.code, self.what = code, what


class NotCovered(MisoError):
    """MISO_E_UNSUPPORTED, before any launch: what a caller with another path for the shape catches, and nothing else."""


def check(rc: int, what: str):
    if rc != 0:
        msg = load().miso_error_string(rc).decode()
        raise (NotCovered if rc == E_UNSUPPORTED else MisoError)(f"{what} failed: {msg} (code {rc})", rc, what)
