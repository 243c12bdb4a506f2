"""Sphere tracing through hash-indexed levels (include/miso_hash_trace.h), everything that needs no GPU: the header
against the binding and against gcc, miso_hash_trace_supported against miso_hash_sdf_supported over the fused kernels'
shape table, the refusals of the launching entry, and what GridNet.sphere_trace declines on the host."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import hash_cases as hc
import test_hash_sdf_host as base

ROOT = base.ROOT
HEADER = os.path.join(ROOT, "include", "miso_hash_trace.h")
E_BADARG, E_UNSUPPORTED, E_TOOLARGE = 2001, 2002, 2003
ENTRIES = ["miso_hash_sphere_trace", "miso_hash_trace_supported"]


# --------------------------------------------------------------------------- #
# include/miso_hash_trace.h
# --------------------------------------------------------------------------- #
def test_header_parses_into_tables_of_its_own():
    from miso_amd import _lib
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(miso_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.HASH_TRACE_SIGNATURES) == ENTRIES
    assert _lib.HASH_TRACE_STRUCTS == {} and _lib.HASH_TRACE_CONSTANTS == {}          # function declarations only
    assert "MISO_HASH_TRACE_H" in text
    # disjoint from the other three headers' tables, which hold what they held
    for other in (_lib.SIGNATURES, _lib.HASH_SIGNATURES, _lib.HASH_SDF_SIGNATURES):
        assert not set(_lib.HASH_TRACE_SIGNATURES) & set(other)
    both = ({**_lib.CONSTANTS, **_lib.HASH_CONSTANTS}, {**_lib.STRUCTS, **_lib.HASH_STRUCTS})
    read = lambda name, b: set(_lib.read_header(open(os.path.join(ROOT, "include", name)).read(), base=b)[2])   # noqa: E731
    assert read("miso_hip.h", None) == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 88
    assert read("miso_hash.h", (_lib.CONSTANTS, _lib.STRUCTS)) == set(_lib.HASH_SIGNATURES) and len(_lib.HASH_SIGNATURES) == 3
    assert read("miso_hash_sdf.h", both) == set(_lib.HASH_SDF_SIGNATURES) == set(base.ENTRIES)
    # it needs both headers' types: miso_mlp_t is miso_hip.h's, miso_hash_grid_t miso_hash.h's
    for b in (None, (_lib.CONSTANTS, _lib.STRUCTS), (_lib.HASH_CONSTANTS, _lib.HASH_STRUCTS)):
        with pytest.raises(_lib.HeaderError):
            _lib.read_header(text, base=b)
    assert sorted(_lib.read_header(text, base=both)[2]) == ENTRIES
    at = text.rindex("#ifdef __cplusplus")
    for extra in ("long miso_x(long);", "#define MISO_X (1 << 3)", "#pragma pack(1)"):
        with pytest.raises(_lib.HeaderError):
            _lib.read_header(text[:at] + extra + "\n" + text[at:], base=both)
    # the binding's view of the launching entry: the argument list of the header, widths included
    res, args = _lib.HASH_TRACE_SIGNATURES["miso_hash_sphere_trace"]
    f, i32, i64, u32, p = ctypes.c_float, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p
    assert res is ctypes.c_int and args[2:] == [p, u32, p, p, i64, f, f, i32, f, f, p, p, p, p, p, p] and len(args) == 18


def test_symbols_are_exported():
    from miso_amd import _lib
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert hasattr(raw, n), f"{n} declared in miso_hash_trace.h but not exported"


def test_header_compiles_as_c_under_werror(tmp_path):
    src, out = tmp_path / "inc.c", tmp_path / "inc.out"
    src.write_text('#include "miso_hash_trace.h"\n#include "miso_hash_trace.h"\n'
                   "int main(void) { return (int)sizeof(miso_hash_grid_t) == 0; }\n")
    run = subprocess.run(["gcc", "-Werror", "-Wall", "-Wextra", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                          "-o", str(out)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


# --------------------------------------------------------------------------- #
# miso_hash_trace_supported (host logic: the table pointers are never dereferenced)
# --------------------------------------------------------------------------- #
def test_supported_agrees_with_the_fused_sdf_query():
    """No shape of the fused table was left out (every instantiation of hash_trace_kernel fits its registers without
    scratch: the table at the top of csrc/hash_trace.hip), so the two answers agree everywhere."""
    from miso_amd import _lib
    lib = _lib.load()
    ref = lambda s: None if s is None else ctypes.byref(s)                                                 # noqa: E731
    both = lambda g, m: (lib.miso_hash_trace_supported(ref(g), ref(m)), lib.miso_hash_sdf_supported(ref(g), ref(m)))   # noqa: E731
    shapes = base._fused_shapes()
    for log2 in hc.LOG2S:
        for C, L, H, NH in shapes:
            assert both(base._hash_grid(base._DIMS4[:L], log2, C), base._mlp(C * L, H, NH)) == (1, 1), (C, L, H, NH, log2)
    g = base._hash_grid()
    odd = base._mlp(8)
    odd.out_dim = 3
    bad_rows, bad_flags = base._hash_grid(), base._hash_grid()
    bad_rows.level[1].rows = 128
    bad_flags.flags = 128
    declined = [(None, base._mlp(8)), (g, None), (base._hash_grid(C=1), base._mlp(2)), (base._hash_grid(C=2), base._mlp(4)),
                (base._hash_grid(C=(4, 8)), base._mlp(12)), (g, base._mlp(8, H=48)), (g, base._mlp(8, NH=2)),
                (g, base._mlp(8, NH=0)), (g, base._mlp(12)), (g, base._mlp(4)), (g, odd), (bad_rows, base._mlp(8)),
                (bad_flags, base._mlp(8))]
    for k, (gg, mm) in enumerate(declined):
        assert both(gg, mm) == (0, 0), k


# --------------------------------------------------------------------------- #
# refusals (host pointers: replayed on machines without a GPU only, as tests/test_hash_sdf_host.py's are)
# --------------------------------------------------------------------------- #
@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="replayed on machines without a GPU only: the cases hand the library HOST pointers, and a "
                           "refusal that had regressed would launch a kernel on them -- never on a shared card")
def test_entry_point_refuses_before_any_launch():
    from miso_amd import _lib
    lib = _lib.load()
    keep = [torch.zeros(64) for _ in range(8)]
    packed, o, d, pts, hit, sdf, steps, grad = (ctypes.c_void_p(t.data_ptr()) for t in keep)
    assert packed.value % 16 == 0
    g, m = base._hash_grid(), base._mlp(8)
    good = dict(grid=g, mlp=m, packed=packed, flags=0, origins=o, dirs=d, n=4, min_dist=1e-3, max_dist=1.0, max_iters=10,
                epsilon=1e-4, fd_step=0.0, points=pts, hit=hit, sdf=None, steps=None, grad=None, stream=None)

    def call(**over):
        a = {**good, **over}
        a["grid"] = None if a["grid"] is None else ctypes.byref(a["grid"])
        a["mlp"] = None if a["mlp"] is None else ctypes.byref(a["mlp"])
        return lib.miso_hash_sphere_trace(*a.values())

    # n < 0, a NULL required pointer with n > 0, a misaligned weight pack
    assert call(n=-1) == E_BADARG
    for name in ("grid", "mlp", "packed", "origins", "dirs", "points", "hit"):
        assert call(**{name: None}) == E_BADARG, name
    for b in (4, 8):
        assert call(packed=ctypes.c_void_p(packed.value + b)) == E_BADARG
    # decoder_flags: 0 or MISO_F_EXACT_F32 and no other bit
    for flags in (1, 2, 4, 64, 256, _lib.F_EXACT_F32 | 1, 1 << 31):
        assert call(flags=flags) == E_BADARG, flags
    # the loop constants
    for it in (0, -1):
        assert call(max_iters=it) == E_BADARG
    for h in (0.0, -1e-2, float("nan"), float("inf")):
        assert call(grad=grad, fd_step=h) == E_BADARG, h
    # a grid that convert_hash_grid refuses: that call's code
    for change in (lambda x: setattr(x, "flags", _lib.F_EXACT_F32), lambda x: setattr(x.level[1], "rows", 128),
                   lambda x: setattr(x.level[0], "table", None)):
        bad = base._hash_grid()
        change(bad)
        assert call(grid=bad) == E_BADARG
    # mixed C, shapes outside the fused table
    for gg, mm in ((base._hash_grid(C=2), base._mlp(4)), (base._hash_grid(C=(4, 8)), base._mlp(12)), (g, base._mlp(8, H=48)),
                   (g, base._mlp(12)), (g, base._mlp(8, NH=2))):
        assert call(grid=gg, mlp=mm) == E_UNSUPPORTED
    # more rays than the launches of this family index
    assert call(n=1 << 40) == E_TOOLARGE
    # n == 0 is served without a launch, whatever the per-ray pointers are
    none = dict(origins=None, dirs=None, points=None, hit=None, packed=None)
    assert call(n=0, **none) == 0
    assert call(n=0, flags=_lib.F_EXACT_F32, grad=grad, fd_step=1e-2, sdf=sdf, steps=steps) == 0
    assert call(n=0, flags=2) == E_BADARG and call(n=0, max_iters=0) == E_BADARG
    assert call(n=0, mlp=base._mlp(8, H=48)) == E_UNSUPPORTED


# --------------------------------------------------------------------------- #
# GridNet.sphere_trace: what declines on the host
# --------------------------------------------------------------------------- #
def test_gridnet_routing_on_the_host():
    from miso_amd import ops
    from miso_amd.grid_opt.models.grid_net import GridNet
    o = torch.tensor([[0.0, 0.0, 0.5]]).repeat(5, 1)
    d = torch.tensor([[0.0, 0.0, 1.0]]).repeat(5, 1)
    on, off, absent = (GridNet(base._cfg(v), device="cpu") for v in (True, False, None))
    reg = base._cfg(True)
    reg["grid"]["type"] = "regular"
    reg = GridNet(reg, device="cpu")
    assert reg._fused_hash_decoder() is None                       # no meaning for a regular grid
    assert off._fused_hash_decoder() is None and absent._fused_hash_decoder() is None      # switch off, switch absent
    for net in (on, off, absent, reg):
        with torch.no_grad():
            assert net.sphere_trace(o, d) is None                  # host tensors
        assert net.sphere_trace(o, d) is None                      # autograd on
    # the ops themselves on host tensors
    import sampler_cases as sc
    meta = ops.GridMeta.from_bound(sc.BOUNDS[hc.BOUND])
    lin = [torch.nn.Linear(8, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 1)]
    pack = ops.DecoderPack([l.weight.detach() for l in lin], [l.bias.detach() for l in lin])
    assert not ops.hash_trace_supported(hc.tables(6, 4), meta, hc.DIMS, 6, pack)
    kw = dict(min_dist=1e-3, max_dist=1.0, max_iters=4, epsilon=1e-4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.hash_sphere_trace(hc.tables(6, 4), meta, hc.DIMS, 6, pack, o, d, **kw)
    with pytest.raises(ValueError, match="max_iters"):
        ops.hash_sphere_trace(hc.tables(6, 4), meta, hc.DIMS, 6, pack, o, d, **dict(kw, max_iters=0))
