"""The fused SDF query of hash-indexed levels (include/miso_hash_sdf.h), everything that needs no GPU: the header
against the binding and against gcc, miso_hash_sdf_supported over the fused kernels' shape table, the refusals of the
two launching entries, and the host logic of GridNet's grid.hash_fused switch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import hash_cases as hc
import sampler_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "miso_hash_sdf.h")
E_BADARG, E_UNSUPPORTED = 2001, 2002
ENTRIES = ["miso_hash_sdf_bwd", "miso_hash_sdf_bwd_workspace_floats", "miso_hash_sdf_fwd", "miso_hash_sdf_supported"]


def _fused_shapes():
    """(C, L, H, NH) of MISO_FUSED_SHAPES, read off csrc/sdf_fused.hpp"""
    text = open(os.path.join(ROOT, "miso_amd", "csrc", "sdf_fused.hpp")).read()
    body = text[text.index("#define MISO_FUSED_SHAPES(X)"):text.index("template <int C, int L, int H, int NH>")]
    shapes = [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", body)]
    assert len(shapes) >= 11 and {s[0] for s in shapes} == {4, 8}
    return shapes


# --------------------------------------------------------------------------- #
# include/miso_hash_sdf.h
# --------------------------------------------------------------------------- #
def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_parses_into_tables_of_its_own():
    from miso_amd import _lib
    names = sorted(set(re.findall(r"\b(miso_[a-z0-9_]+)\s*\(", _header_code())))
    assert names == sorted(_lib.HASH_SDF_SIGNATURES) == ENTRIES
    assert _lib.HASH_SDF_STRUCTS == {} and _lib.HASH_SDF_CONSTANTS == {}            # function declarations only
    assert "MISO_HASH_SDF_H" in open(HEADER).read()
    # disjoint from the other two headers' tables, which hold what they held
    for other in (_lib.SIGNATURES, _lib.HASH_SIGNATURES):
        assert not set(_lib.HASH_SDF_SIGNATURES) & set(other)
    hip = open(os.path.join(ROOT, "include", "miso_hip.h")).read()
    assert set(_lib.read_header(hip)[2]) == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 88
    hsh = open(os.path.join(ROOT, "include", "miso_hash.h")).read()
    assert set(_lib.read_header(hsh, base=(_lib.CONSTANTS, _lib.STRUCTS))[2]) == set(_lib.HASH_SIGNATURES) == \
        {"miso_hash_rows", "miso_hash_encode_fwd", "miso_hash_encode_bwd"}
    # it needs both headers' types: miso_mlp_t is miso_hip.h's, miso_hash_grid_t miso_hash.h's
    text = open(HEADER).read()
    for base in (None, (_lib.CONSTANTS, _lib.STRUCTS), (_lib.HASH_CONSTANTS, _lib.HASH_STRUCTS)):
        with pytest.raises(_lib.HeaderError):
            _lib.read_header(text, base=base)
    both = ({**_lib.CONSTANTS, **_lib.HASH_CONSTANTS}, {**_lib.STRUCTS, **_lib.HASH_STRUCTS})
    assert sorted(_lib.read_header(text, base=both)[2]) == ENTRIES
    at = text.rindex("#ifdef __cplusplus")
    for extra in ("long miso_x(long);", "#define MISO_X (1 << 3)", "#pragma pack(1)"):
        with pytest.raises(_lib.HeaderError):
            _lib.read_header(text[:at] + extra + "\n" + text[at:], base=both)


def test_symbols_are_exported():
    from miso_amd import _lib
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in _lib.HASH_SDF_SIGNATURES:
        assert hasattr(raw, n), f"{n} declared in miso_hash_sdf.h but not exported"


def _gcc(tmp_path, name, text, *flags):
    src, out = tmp_path / name, tmp_path / (name + ".out")
    src.write_text(text)
    run = subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(out)],
                         capture_output=True, text=True)
    return run, out


def test_header_compiles_as_c_under_werror(tmp_path):
    run, _ = _gcc(tmp_path, "inc.c", '#include "miso_hash_sdf.h"\n#include "miso_hash_sdf.h"\n'
                  "int main(void) { return (int)sizeof(miso_hash_grid_t) == 0; }\n", "-Wall", "-Wextra", "-std=c99")
    assert run.returncode == 0, run.stderr


_SIG_PRELUDE = """#include <type_traits>
#include "miso_hash_sdf.h"
template <class T> struct arg { using type = T; };
template <class T> struct arg<T*> {
  using U = std::remove_cv_t<T>;
  using type = std::conditional_t<std::is_class_v<U> || std::is_same_v<U, char>, U, void>*;
};
template <class F> struct abi;
template <class R, class... A> struct abi<R(A...)> { using type = typename arg<R>::type(typename arg<A>::type...); };
"""
_C_SCALARS = {"i": "int", "I": "unsigned int", "l": "long", "L": "unsigned long", "f": "float", "d": "double", "P": "void*"}


def test_prototypes_equal_the_binding_as_a_cxx_compiler_sees_them(tmp_path):
    """tests/test_hash_host.py's scheme: each declared function's type (a scalar stays itself, a pointer to a miso struct
    keeps the struct, every other pointer is void*) against the type spelled from the binding's restype / argtypes; a
    binding with a narrowed argument must be refused."""
    from miso_amd import _lib
    names = {c: n for n, c in {**_lib.STRUCTS, **_lib.HASH_STRUCTS}.items()}

    def spell(t):
        return names[t._type_] + "*" if hasattr(t, "contents") else _C_SCALARS[t._type_]

    def accepted(name, signatures):
        text = _SIG_PRELUDE + "".join(
            f'static_assert(std::is_same_v<abi<decltype({n})>::type, {spell(res)}({", ".join(map(spell, args))})>, "{n}");\n'
            for n, (res, args) in signatures.items())
        run, _ = _gcc(tmp_path, name, text, "-x", "c++", "-std=c++17", "-c")
        return run.returncode == 0, run.stderr

    sigs = _lib.HASH_SDF_SIGNATURES
    ok, err = accepted("sig.cpp", sigs)
    assert ok, err
    res, args = sigs["miso_hash_sdf_fwd"]
    assert args[3] is ctypes.c_uint32 and args[5] is ctypes.c_int64
    ok, err = accepted("narrow.cpp", {**sigs, "miso_hash_sdf_fwd": (res, args[:5] + [ctypes.c_int32] + args[6:])})
    assert not ok and "static assertion failed" in err, err
    assert sigs["miso_hash_sdf_bwd_workspace_floats"][0] is ctypes.c_int64


# --------------------------------------------------------------------------- #
# miso_hash_sdf_supported (host logic: the table pointers are never dereferenced)
# --------------------------------------------------------------------------- #
_DIMS4 = hc.DIMS + ((9, 4, 11), (6, 6, 6))


def _hash_grid(dims=hc.DIMS, log2=6, C=4):
    from miso_amd import _lib
    g = _lib.HashGrid()
    g.n_levels = len(dims)
    for a in range(3):
        g.bound_min[a], g.bound_max[a] = -1.0, 1.0
    for l, d in enumerate(dims):
        rows, dense = hc.level_rows(d, log2)
        lv = g.level[l]
        lv.table, lv.rows, lv.C = 4096, rows, C if isinstance(C, int) else C[l]      # a dummy aligned non-NULL pointer
        lv.X, lv.Y, lv.Z = d
        lv.log2_rows = 0 if dense else log2
    return g


def _mlp(in_dim, H=64, NH=1):
    from miso_amd import _lib
    m = _lib.Mlp()
    m.n_linear, m.in_dim, m.hidden_dim, m.out_dim = NH + 2, in_dim, H, 1
    return m


def test_supported_is_the_fused_shape_table():
    from miso_amd import _lib
    lib = _lib.load()
    sup = lambda g, m: lib.miso_hash_sdf_supported(None if g is None else ctypes.byref(g), None if m is None else ctypes.byref(m))
    for log2 in hc.LOG2S:
        for C, L, H, NH in _fused_shapes():
            assert sup(_hash_grid(_DIMS4[:L], log2, C), _mlp(C * L, H, NH)) == 1, (C, L, H, NH, log2)
    g = _hash_grid()
    assert sup(g, _mlp(8)) == 1
    assert lib.miso_hash_sdf_bwd_workspace_floats(ctypes.byref(g), 257) == 257 * 8
    assert lib.miso_hash_sdf_bwd_workspace_floats(ctypes.byref(g), 0) == 0
    assert sup(None, _mlp(8)) == 0 and sup(g, None) == 0
    for C in (1, 2):
        assert sup(_hash_grid(C=C), _mlp(2 * C)) == 0
    assert sup(_hash_grid(C=(4, 8)), _mlp(12)) == 0                      # mixed C
    assert sup(g, _mlp(8, H=48)) == 0
    assert sup(g, _mlp(8, NH=2)) == 0 and sup(g, _mlp(8, NH=0)) == 0     # depths outside the table
    assert sup(g, _mlp(12)) == 0 and sup(g, _mlp(4)) == 0                # input width is not C * L
    m = _mlp(8)
    m.out_dim = 3
    assert sup(g, m) == 0
    bad = _hash_grid()
    bad.level[1].rows = 128                                              # rows disagree with the level's shape
    assert sup(bad, _mlp(8)) == 0 and lib.miso_hash_sdf_bwd_workspace_floats(ctypes.byref(bad), 4) == 0
    bad = _hash_grid()
    bad.flags = 128                                                      # the decoder arithmetic is not a grid flag here
    assert sup(bad, _mlp(8)) == 0


# --------------------------------------------------------------------------- #
# refusals (host pointers: replayed on machines without a GPU only, as tests/test_hash_host.py's are)
# --------------------------------------------------------------------------- #
@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="replayed on machines without a GPU only: the cases hand the library HOST pointers, and a "
                           "refusal that had regressed would launch a kernel on them -- never on a shared card")
def test_entry_points_refuse_before_any_launch():
    from miso_amd import _lib
    lib = _lib.load()
    n = 4
    keep = [torch.zeros(64) for _ in range(7)]
    packed, x, sdf, gsdf, mask, ws, gx = (ctypes.c_void_p(t.data_ptr()) for t in keep)
    assert all(p.value % 16 == 0 for p in (packed, ws))

    def fwd(g, m, packed=packed, flags=0, x=x, n=n, sdf=sdf, mask=mask):
        return lib.miso_hash_sdf_fwd(None if g is None else ctypes.byref(g), None if m is None else ctypes.byref(m), packed,
                                     flags, x, n, sdf, mask, None)

    def bwd(g, m, packed=packed, flags=0, x=x, n=n, gsdf=gsdf, mask=mask, gx=None, ws=ws):
        return lib.miso_hash_sdf_bwd(None if g is None else ctypes.byref(g), None if m is None else ctypes.byref(m), packed,
                                     flags, x, n, gsdf, mask, gx, ws, None)

    g, m = _hash_grid(), _mlp(8)
    # NULL arguments with n > 0
    for kw in ({"packed": None}, {"x": None}, {"sdf": None}):
        assert fwd(g, m, **kw) == E_BADARG, kw
    for kw in ({"packed": None}, {"x": None}, {"gsdf": None}, {"mask": None}, {"ws": None}):
        assert bwd(g, m, **kw) == E_BADARG, kw
    assert fwd(None, m) == E_BADARG and bwd(None, m) == E_BADARG and fwd(g, None) == E_BADARG and bwd(g, None) == E_BADARG
    assert fwd(g, m, n=-1) == E_BADARG and bwd(g, m, n=-1) == E_BADARG
    # decoder_flags: 0 or MISO_F_EXACT_F32 and no other bit
    for flags in (1, 2, 4, 64, 256, _lib.F_EXACT_F32 | 1, 1 << 31):
        assert fwd(g, m, flags=flags) == E_BADARG and bwd(g, m, flags=flags) == E_BADARG, flags
    # alignment: the workspace and the packed weights are read and written 16 bytes at a time
    off = lambda p, b: ctypes.c_void_p(p.value + b)      # noqa: E731
    for b in (4, 8):
        assert bwd(g, m, ws=off(ws, b)) == E_BADARG
        assert fwd(g, m, packed=off(packed, b)) == E_BADARG and bwd(g, m, packed=off(packed, b)) == E_BADARG
    # the grid's own checks are miso_hash_encode_fwd's, the decoder arithmetic is not among its flags
    bad = _hash_grid()
    bad.flags = _lib.F_EXACT_F32
    assert fwd(bad, m) == E_BADARG and bwd(bad, m) == E_BADARG
    bad = _hash_grid()
    bad.level[1].rows = 128
    assert fwd(bad, m) == E_BADARG and bwd(bad, m) == E_BADARG
    bad = _hash_grid()
    bad.level[0].table = None                            # the forward reads every table; the backward only for grad_x
    assert fwd(bad, m) == E_BADARG and bwd(bad, m, gx=gx) == E_BADARG
    # shapes outside the table
    for gg, mm in ((_hash_grid(C=2), _mlp(4)), (_hash_grid(C=(4, 8)), _mlp(12)), (g, _mlp(8, H=48)), (g, _mlp(12)),
                   (g, _mlp(8, NH=2))):
        assert fwd(gg, mm) == E_UNSUPPORTED and bwd(gg, mm) == E_UNSUPPORTED
    # n == 0 is served without a launch, whatever the per-point pointers are
    assert fwd(g, m, n=0, x=None, sdf=None, mask=None, packed=None) == 0
    assert bwd(g, m, n=0, x=None, gsdf=None, mask=None, ws=None, packed=None) == 0
    assert fwd(g, m, n=0, flags=_lib.F_EXACT_F32) == 0 and bwd(g, m, n=0, flags=_lib.F_EXACT_F32) == 0
    assert fwd(g, m, n=0, flags=2) == E_BADARG and fwd(g, _mlp(8, H=48), n=0) == E_UNSUPPORTED


# --------------------------------------------------------------------------- #
# GridNet: the switch on the host
# --------------------------------------------------------------------------- #
BOUND = [[-1.0, 1.3], [-0.7, 0.9], [0.0, 2.1]]


def _cfg(hash_fused=None):
    import golden_cases as gc
    cfg = gc.model_cfg(BOUND, 0.5, 2.0, 2, 4, 64, num_poses=2, init_stddev=0.01)
    cfg["grid"]["type"] = "hash"
    cfg["grid"]["log2_hashmap_size"] = 8
    if hash_fused is not None:
        cfg["grid"]["hash_fused"] = hash_fused
    return cfg


def test_gridnet_switch_on_the_host():
    from miso_amd import ops
    from miso_amd.grid_opt.models.grid_net import GridNet
    net = GridNet(_cfg(True), device="cpu")
    assert net.hash_fused is True and net.decoder.decoder_pack() is not None
    assert net._fused_hash_decoder() is None and net._fused_decoder() is None      # host tensors: no fused route
    assert GridNet(_cfg(), device="cpu").hash_fused is False                       # key absent
    assert GridNet(_cfg(False), device="cpu").hash_fused is False
    assert GridNet(_cfg(), device="cpu")._fused_hash_decoder() is None
    reg = _cfg(True)
    reg["grid"]["type"] = "regular"
    assert GridNet(reg, device="cpu")._fused_hash_decoder() is None                # no meaning for a regular grid
    # the op itself on host tensors
    meta = ops.GridMeta.from_bound(sc.BOUNDS[hc.BOUND])
    lin = [torch.nn.Linear(8, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 1)]
    pack = ops.DecoderPack([l.weight.detach() for l in lin], [l.bias.detach() for l in lin])
    assert not ops.hash_sdf_supported(hc.tables(6, 4), meta, hc.DIMS, 6, pack)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.hash_sdf_fused(torch.zeros(5, 3), hc.tables(6, 4), meta, hc.DIMS, 6, pack)
