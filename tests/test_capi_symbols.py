"""CPU-side checks of the drop-in boundary: the shared library loads and exports
every symbol include/miso_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_code():
    src = open(os.path.join(ROOT, "include", "miso_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(miso_[a-z0-9_]+)\s*\(", _header_code())))


def test_library_exports_every_declared_symbol():
    from miso_amd import _lib
    names = _declared()
    assert len(names) >= 12
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in miso_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in miso_amd/_lib.py"
    assert set(_lib.SIGNATURES) == set(names)
    assert b"gfx950" in lib.miso_version()
    # the library was built from THIS tree: miso_version() embeds a hash of the kernel sources
    import importlib.util
    spec = importlib.util.spec_from_file_location("srchash", os.path.join(ROOT, "miso_amd", "csrc", "srchash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert lib.miso_version().decode().endswith("src=" + mod.source_hash()), \
        "libmiso_hip.so is stale: rebuild with `make -C miso_amd/csrc`"
    assert lib.miso_error_string(2001) == b"bad argument"


def test_struct_layout_matches_header():
    from miso_amd import _lib
    # sizes implied by the C declarations (LP64)
    assert ctypes.sizeof(_lib.Level) == 8 + 8 + 4 * 4 + 8 * 4 + 8      # ... + grad_touched
    assert ctypes.sizeof(_lib.Grid) == 4 + 4 + 12 + 12 + 4 + 4 + 8 * ctypes.sizeof(_lib.Level)
    assert ctypes.sizeof(_lib.Mlp) == 16 + 8 * 4 + 8 * 4


def test_ops_refuse_cpu_tensors():
    """No silent CPU fallback: the product ops raise on CPU tensors."""
    from miso_amd import ops
    f = torch.zeros(1, 4, 3, 3, 3)
    x = torch.zeros(5, 3)
    meta = ops.GridMeta.from_bound([[-1, 1]] * 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.encode(x, [f], meta)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.adam_dense_(f, f.clone(), f.clone(), f.clone(), 1, 1e-3)


def test_argument_validation_without_gpu():
    """Entry points validate arguments before touching the device."""
    from miso_amd import _lib
    lib = _lib.load()
    g = _lib.Grid()
    g.n_levels = 0
    assert lib.miso_encode_fwd(ctypes.byref(g), None, None, 0, None, 0, None) == 2001
    g.n_levels = 1
    g.level[0].C = 4; g.level[0].X = 2; g.level[0].Y = 2; g.level[0].Z = 2
    g.level[0].sC = 1; g.level[0].sX = 4; g.level[0].sY = 8; g.level[0].sZ = 16
    assert lib.miso_encode_fwd(ctypes.byref(g), None, None, 0, None, 4, None) == 2001  # data NULL
    g.flags = 128
    assert lib.miso_encode_fwd(ctypes.byref(g), None, None, 0, None, 4, None) == 2001  # bad flag
    m = _lib.Mlp()
    m.in_dim, m.hidden_dim, m.out_dim, m.n_linear = 24, 64, 1, 3
    assert lib.miso_mlp_packed_floats(ctypes.byref(m)) > 0
    assert lib.miso_sdf_mask_words(ctypes.byref(m)) == 4
    m.hidden_dim = 48
    assert lib.miso_mlp_packed_floats(ctypes.byref(m)) == 0


def test_refusals_are_typed_without_gpu():
    """_lib.check turns MISO_E_UNSUPPORTED into NotCovered and every other code into a plain MisoError, the message as
    it always was; a decoder the library does not pack is NotCovered for a caller that demands it (require) and
    (None, None) for one that asks (get) -- decided by host code, so on host tensors too."""
    from miso_amd import _lib, ops
    assert ops.NotCovered is _lib.NotCovered and ops.MisoError is _lib.MisoError
    assert issubclass(_lib.NotCovered, _lib.MisoError) and issubclass(_lib.MisoError, RuntimeError)
    with pytest.raises(_lib.NotCovered) as e:
        _lib.check(_lib.E_UNSUPPORTED, "x")
    assert e.value.code == _lib.E_UNSUPPORTED == 2002 and e.value.what == "x"
    assert str(e.value) == "x failed: shape not covered by the fused kernels (code 2002)"
    with pytest.raises(_lib.MisoError) as e:
        _lib.check(_lib.E_BADARG, "x")
    assert not isinstance(e.value, _lib.NotCovered) and e.value.code == 2001
    assert str(e.value) == "x failed: bad argument (code 2001)"
    assert _lib.check(0, "x") is None
    pack = ops.DecoderPack([torch.zeros(48, 12), torch.zeros(48, 48), torch.zeros(1, 48)], [None, None, None])
    with pytest.raises(ops.NotCovered, match="decoder shape is not covered by the fused kernels") as e:
        pack.require()
    assert e.value.code == _lib.E_UNSUPPORTED
    assert pack.get() == (None, None)
    # a decoder that would pack is still refused on the host for what it is: no device
    ok = ops.DecoderPack([torch.zeros(64, 24), torch.zeros(64, 64), torch.zeros(1, 64)], [None, None, None])
    for _ in range(2):
        with pytest.raises(RuntimeError, match="HIP device only"):
            ok.get()


def test_round2_entry_points_validate_arguments_without_gpu():
    """The entry points added for the captured trainer step, the tracker and the batch prologue refuse bad arguments
    before any launch; miso_adam_scalars_table is a host function and can be checked against the formula here."""
    import math
    from miso_amd import _lib
    lib = _lib.load()
    E = 2001
    # step scalars: {1 - b1, b2, 1 - b2, -lr / (1 - b1^t), sqrt(1 - b2^t), eps} as torch.optim.Adam computes them
    host = torch.empty((4, 6), dtype=torch.float32)
    assert lib.miso_adam_scalars_table(1e-3, 0.9, 0.999, 1e-8, 1, 4, ctypes.c_void_p(host.data_ptr())) == 0
    for t in range(1, 5):
        want = [1 - 0.9, 0.999, 1 - 0.999, -(1e-3 / (1 - 0.9 ** t)), math.sqrt(1 - 0.999 ** t), 1e-8]
        assert torch.allclose(host[t - 1], torch.tensor(want, dtype=torch.float32), rtol=1e-6, atol=0)
    assert lib.miso_adam_scalars_table(1e-3, 0.9, 0.999, 1e-8, 0, 4, ctypes.c_void_p(host.data_ptr())) == E
    assert lib.miso_adam_scalars_table(1e-3, 0.9, 0.999, 1e-8, 1, 4, None) == E
    assert lib.miso_adam_bump(None, None, None) == E
    tensor, when = _lib.AdamTensor(), _lib.AdamWhen()
    tensor.numel, when.table_len = 8, 1                      # no arrays; a table length without table or count
    assert lib.miso_adam_step(ctypes.byref(tensor), 1, ctypes.byref(when), None, None) == E
    when.lr, when.beta1, when.beta2, when.eps, when.step, when.table_len = 1e-3, 0.9, 0.999, 1e-8, 1, 0
    assert lib.miso_adam_step(ctypes.byref(tensor), 1, ctypes.byref(when), None, None) == E          # no arrays
    tensor.numel, when.step = 0, 0
    assert lib.miso_adam_step(ctypes.byref(tensor), 1, ctypes.byref(when), None, None) == E          # step 0
    assert lib.miso_adam_step(None, 1, ctypes.byref(when), None, None) == E
    assert lib.miso_adam_step(ctypes.byref(tensor), 1, None, None, None) == E
    assert lib.miso_mapping_batch(None, None, 1, None, 1, None, None, None, None, None, None, None, 0, 0, None, None, 0, None) == E
    assert lib.miso_mapping_loss_rows(7, 1.0, 0.0, 0.0, None, None, 0, None, None, None) == E
    assert lib.miso_mapping_loss_rows(1, 1.0, 0.0, 0.0, None, None, 4, None, None, None) == E
    assert lib.miso_lm_track_step(None, None, None, None, None) == E
    assert lib.miso_track_adam_step(None, None, None, None, None) == E
    a = _lib.LmTrack()
    g = _lib.Grid()
    g.n_levels = 1
    assert lib.miso_lm_track_step(ctypes.byref(g), None, None, ctypes.byref(a), None) == E      # no pose pointers
    t = _lib.TrackAdam()
    assert lib.miso_track_adam_step(ctypes.byref(g), None, None, ctypes.byref(t), None) == E


def test_gradient_plans_are_host_logic(monkeypatch):
    """Which levels the binned backward pulls, pushes or scatters is decided on the host from the grid shape, the batch
    size and the flags (miso_grad_pull_levels / miso_sdf_bwd_push_levels): no device call, so it is checked here."""
    from miso_amd import _lib
    lib = _lib.load()

    def grid(sizes, C, flags=0):
        g = _lib.Grid()
        g.n_levels = len(sizes)
        g.flags = flags
        for a in range(3):
            g.bound_min[a], g.bound_max[a] = -1.0, 1.0
        for l, (x, y, z) in enumerate(sizes):
            lv = g.level[l]
            lv.C, lv.X, lv.Y, lv.Z = C, x, y, z
            lv.sC, lv.sX, lv.sY, lv.sZ = 1, C, C * x, C * x * y          # channels-last
            lv.data = None
            lv.grad = 0x100000 * (l + 1)                                 # never dereferenced by the planners
        return g

    T = 16
    cfg2 = grid([(32, 32, 32), (64, 64, 64), (128, 128, 128)], 8)
    assert lib.miso_grad_pull_levels(ctypes.byref(cfg2), T) == 0b111
    assert lib.miso_sdf_bwd_push_levels(ctypes.byref(cfg2), T, 262144) == 0          # 64 samples a tile: pulled
    scannet = grid([(40, 20, 40), (200, 100, 200)], 4)
    assert lib.miso_grad_pull_levels(ctypes.byref(scannet), T) == 0b01                # 13 x 7 x 13 bricks: scattered
    assert lib.miso_sdf_bwd_push_levels(ctypes.byref(scannet), T, 540000) == 0b01     # a crowd on the coarse level
    assert lib.miso_sdf_bwd_push_levels(ctypes.byref(scannet), T, 54000) == 0
    crowded = grid([(40, 20, 40), (200, 100, 200)], 4, flags=_lib.F_CROWDED)
    assert lib.miso_sdf_bwd_push_levels(ctypes.byref(crowded), T, 54000) == 0b01      # the caller's hint
    assert lib.miso_sdf_bwd_push_levels(ctypes.byref(crowded), T, 1000) == 0
    ncd = grid([(120, 120, 20), (600, 600, 100)], 4)
    assert lib.miso_grad_pull_levels(ctypes.byref(ncd), T) == 0b01                   # 38 vertices per tile and axis
    border = grid([(32, 32, 32)], 8, flags=2)                                         # padding_mode='border'
    assert lib.miso_grad_pull_levels(ctypes.byref(border), T) == 0

    # One plan (csrc/grad_plan.hip) answers all four queries.  The values below were read from the library before the
    # plan existed and are pinned as literals.
    from miso_amd import ops
    pulled, pushed = lib.miso_grad_pull_levels, lib.miso_sdf_bwd_push_levels
    scattered, on_mc = lib.miso_sdf_bwd_scattered_levels, lib.miso_grad_pull_on_matrix_cores
    pyramid = grid([(16,) * 3, (32,) * 3, (48,) * 3, (64,) * 3, (128,) * 3], 4)
    assert pulled(ctypes.byref(pyramid), T) == 0b01111                                # PULL_MAXL levels are swept together
    assert scattered(ctypes.byref(pyramid), T, 1000) == 0b10000                       # ... the fifth is scattered
    tiny = grid([(8, 8, 8)], 8)
    assert pulled(ctypes.byref(tiny), T) == 0b1                                        # by the vector kernels:
    assert on_mc(ctypes.byref(tiny), T, 1000, 8) == 0                                  # cells twice as wide as tiles
    assert pulled(ctypes.byref(tiny), ops.pack_tiles((16, 16, 17))) == 0               # ... which serve no per-axis binning
    assert on_mc(ctypes.byref(cfg2), T, 262144, 24) == 1
    assert on_mc(ctypes.byref(cfg2), T, 1 << 26, 24) == 0                              # 6 GB of d-feat rows: 32-bit offsets
    assert on_mc(ctypes.byref(cfg2), T, (1 << 31) // 96 - 1, 24) == 1 and on_mc(ctypes.byref(cfg2), T, (1 << 31) // 96 + 1, 24) == 0
    assert on_mc(ctypes.byref(cfg2), T, 0, 24) == 0                                    # an empty batch
    with monkeypatch.context() as m:
        m.setenv("MISO_PULL_MC", "0")                                                 # read at every call
        assert on_mc(ctypes.byref(cfg2), T, 262144, 24) == 0
        assert pulled(ctypes.byref(cfg2), T) == 0b111
    assert on_mc(ctypes.byref(cfg2), T, 262144, 24) == 1
    ignored = grid([(32, 32, 32), (64, 64, 64), (128, 128, 128)], 8)
    ignored.ignore_mask = 0b010
    assert pulled(ctypes.byref(ignored), T) == 0b111                                  # the pull writes its zeros
    assert scattered(ctypes.byref(ignored), T, 262144) == 0
    for C in (12, 6):                                                                 # no kernel is compiled for them
        odd = grid([(32, 32, 32), (64, 64, 64)], C)
        assert pulled(ctypes.byref(odd), T) == 0 and pushed(ctypes.byref(odd), T, 540000) == 0
        assert scattered(ctypes.byref(odd), T, 540000) == 0b11 and on_mc(ctypes.byref(odd), T, 1000, 2 * C) == 0
    # the crowd threshold: 100 samples a tile on average; a pushed level is added to with atomics, like a scattered one
    for g, n, push, scat in ((scannet, 100 * 4096 - 1, 0, 0b10), (scannet, 100 * 4096, 0b01, 0b11),
                             (crowded, 4096, 0b01, 0b11), (crowded, 4095, 0, 0b10)):
        assert pushed(ctypes.byref(g), T, n) == push and scattered(ctypes.byref(g), T, n) == scat, n
    assert on_mc(ctypes.byref(scannet), T, 100 * 4096 - 1, 8) == 1 and on_mc(ctypes.byref(scannet), T, 100 * 4096, 8) == 0
    # a per-axis binning: bricks of 8 x 7 x 8 on the fine level, everything on the matrix cores, nothing pushed
    xyz = ops.pack_tiles((25, 16, 25))
    assert xyz == 25 | (16 << 8) | (25 << 16)
    assert pulled(ctypes.byref(scannet), xyz) == 0b11 and pushed(ctypes.byref(scannet), xyz, 540000) == 0
    assert scattered(ctypes.byref(scannet), xyz, 540000) == 0 and on_mc(ctypes.byref(scannet), xyz, 540000, 8) == 1
    assert on_mc(ctypes.byref(scannet), xyz, 1 << 26, 8) == 0 and on_mc(ctypes.byref(scannet), xyz, 0, 8) == 0
    assert pulled(ctypes.byref(cfg2), ops.pack_tiles((32, 32, 32))) == 0b111
    assert pulled(ctypes.byref(cfg2), 17) == 0 and scattered(ctypes.byref(cfg2), 17, 1000) == 0      # not a tiles code


def _gcc(tmp_path, name, text, *flags):
    """Compiles `text` against include/miso_hip.h; returns the finished gcc run and the output path."""
    import subprocess
    src, out = tmp_path / name, tmp_path / (name + ".out")
    src.write_text(text)
    run = subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(out)],
                         capture_output=True, text=True)
    return run, out


def test_struct_sizes_and_offsets_equal_the_headers_as_a_c_compiler_sees_it(tmp_path):
    """include/miso_hip.h compiled by gcc: sizeof of EVERY struct of the binding, and offsetof and sizeof of every field
    (a binding that drifts from the header corrupts arguments silently).  The list comes from the binding, which refuses
    a header it reads only in part (test_reader_refuses_what_it_cannot_parse); the struct count is re-checked here."""
    import subprocess
    from miso_amd import _lib
    assert len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", _header_code())) >= 11
    assert _lib.STRUCTS["miso_level_t"] is _lib.Level and _lib.STRUCTS["miso_ray_sampling_t"] is _lib.RaySampling
    probes = []
    for n, c in _lib.STRUCTS.items():
        probes.append((f"sizeof({n})", ctypes.sizeof(c)))
        for f, _ in c._fields_:
            probes.append((f"offsetof({n}, {f})", getattr(c, f).offset))
            probes.append((f"sizeof((({n}*)0)->{f})", getattr(c, f).size))
    body = "".join(f'  printf("%zu\\n", {expr});\n' for expr, _ in probes)
    run, exe = _gcc(tmp_path, "layout.c", '#include <stdio.h>\n#include <stddef.h>\n#include "miso_hip.h"\n'
                    "int main(void) {\n" + body + "  return 0;\n}\n")
    assert run.returncode == 0, run.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(probes)
    wrong = [(expr, g, want) for (expr, want), g in zip(probes, got) if g != want]
    assert not wrong, wrong


# Parameter and return types of every declared function as the compiler sees them, reduced to what a ctypes call can get
# wrong: a scalar stays itself (kind, width, signedness), a pointer to a miso_*_t struct keeps the struct, const char*
# stays a string, every other pointer is void*.  The expected type is spelled from the binding's restype / argtypes.
_SIG_PRELUDE = """#include <type_traits>
#include "miso_hip.h"
template <class T> struct arg { using type = T; };
template <class T> struct arg<T*> {
  using U = std::remove_cv_t<T>;
  using type = std::conditional_t<std::is_class_v<U> || std::is_same_v<U, char>, U, void>*;
};
template <class F> struct abi;
template <class R, class... A> struct abi<R(A...)> { using type = typename arg<R>::type(typename arg<A>::type...); };
"""
_C_SCALARS = {"i": "int", "I": "unsigned int", "l": "long", "L": "unsigned long", "b": "signed char", "B": "unsigned char",
              "f": "float", "d": "double", "P": "void*", "z": "char*"}


def _signature_checks(structs, signatures):
    names = {c: n for n, c in structs.items()}

    def spell(t):
        return names[t._type_] + "*" if hasattr(t, "contents") else _C_SCALARS[t._type_]

    return _SIG_PRELUDE + "".join(
        f'static_assert(std::is_same_v<abi<decltype({n})>::type, {spell(res)}({", ".join(map(spell, args))})>, "{n}");\n'
        for n, (res, args) in signatures.items())


def test_function_signatures_equal_the_headers_as_a_compiler_sees_them(tmp_path):
    """Nothing else checks a function's argument list: a ctypes call with a missing argument, or an int32 where the header
    says int64_t, passes garbage in a register and the kernel runs on it.  gcc (as C++, for the parameter packs) compares
    every prototype of the header with the type spelled from the binding; three wrong bindings must each be refused."""
    from miso_amd import _lib
    C = ctypes

    def accepted(name, signatures):
        run, _ = _gcc(tmp_path, name, _signature_checks(_lib.STRUCTS, signatures), "-x", "c++", "-std=c++17", "-c")
        return run.returncode == 0, run.stderr

    sigs = _lib.SIGNATURES
    assert set(sigs) == set(_declared()) and len(sigs) >= 69
    ok, err = accepted("sig.cpp", sigs)
    assert ok, err

    def mutated(name, change):
        res, args = sigs[name]
        args = list(args)
        change(args)
        return {**sigs, name: (res, args)}

    def to_int32(args):
        assert args[5] is C.c_int64
        args[5] = C.c_int32

    def swap_float_double(args):                      # (lr, beta1 .. eps) are doubles; make the first one a float
        assert args[5] is C.c_double
        args[5] = C.c_float

    wrong = {"dropped.cpp": mutated("miso_atlas_sdf_fwd", lambda a: a.pop()),
             "narrow.cpp": mutated("miso_encode_fwd", to_int32),                              # ld_out
             "float.cpp": mutated("miso_adam_dense", swap_float_double),
             "struct.cpp": mutated("miso_sdf_supported", lambda a: a.__setitem__(1, C.POINTER(_lib.Grid))),
             "return.cpp": {**sigs, "miso_sort_workspace_bytes": (C.c_int32, sigs["miso_sort_workspace_bytes"][1])}}
    for name, bad in wrong.items():
        ok, err = accepted(name, bad)
        assert not ok and "static assertion failed" in err, (name, err)


def test_reader_refuses_what_it_cannot_parse():
    """A declaration the reader skipped would leave a symbol or a struct unbound without a word: it raises instead."""
    from miso_amd import _lib
    header = open(os.path.join(ROOT, "include", "miso_hip.h")).read()
    consts, structs, sigs = _lib.read_header(header)
    assert consts["MISO_MAX_LEVELS"] == _lib.MAX_LEVELS == 8 and set(sigs) == set(_lib.SIGNATURES)
    at = header.rindex("#ifdef __cplusplus")
    for extra in ("typedef union { int a; } u_t;", "long miso_x(long);", "int miso_x(int32_t);", "int miso_x(int a[3]);",
                  "typedef struct { long a; } miso_x_t;", "typedef struct { float* a, b; } miso_x_t;",
                  "typedef struct { int a[MISO_NO_SUCH]; } miso_x_t;", "typedef struct { int a; } other_t;",
                  "#define MISO_X (1 << 3)", "#pragma pack(1)"):
        with pytest.raises(_lib.HeaderError):
            _lib.read_header(header[:at] + extra + "\n" + header[at:])


def test_tile_codes_pack_and_choose():
    """MISO_TILES_XYZ on the Python side (ops.pack_tiles / n_tiles / choose_tiles): a count stays a count, per-axis counts
    are packed as the header's macro packs them, and the policy follows the finest level within what the matrix-core
    pull accepts (3 size >= 2 tiles for every level)."""
    import torch
    from miso_amd import ops
    assert ops.pack_tiles(16) == 16 and ops.pack_tiles((16, 16, 16)) == 16 and ops.n_tiles(16) == 4096
    code = ops.pack_tiles((25, 13, 25))
    assert code == 25 | (13 << 8) | (25 << 16) and ops.n_tiles(code) == 25 * 13 * 25
    assert ops.pack_tiles((32, 32, 32)) == 32 | (32 << 8) | (32 << 16)          # cubic but beyond 16: packed
    f = lambda z, y, x: torch.empty(1, 4, z, y, x)                                # noqa: E731
    assert ops.choose_tiles([f(32, 32, 32), f(128, 128, 128)]) == 16             # cfg-2: 8 vertices per tile already
    assert ops.choose_tiles([f(40, 20, 40), f(200, 100, 200)]) == ops.pack_tiles((25, 16, 25))      # ScanNet submap
    # a coarse level of 16 vertices caps the binning at 24 tiles: the 200-vertex axis cannot be owned, stays at 16
    assert ops.choose_tiles([f(16, 16, 16), f(200, 100, 200)]) == 16
    assert ops.choose_tiles([f(20, 120, 120), f(100, 600, 600)]) == 16           # Newer College: too fine even for 32


def test_train_kernel_lds_fits_for_every_fused_shape():
    """the scattering form of the one-launch training kernel needs the weights + four d-feat tiles + four
    record blocks in LDS; sdf_train_supported routes a shape that would not fit to the two-launch path.  The library
    plans that launch (sdf_train.hip: plan_train) and reports its widest form (miso_sdf_train_lds_bytes); the figures are
    pinned here, and every shape the library instantiates fits 160 KB."""
    from miso_amd import ops
    # MISO_FUSED_SHAPES (sdf_fused.hpp): (C, L, H) -> bytes (scattering, nothing scattered)
    table = {(4, 1, 32): (71056, 38288), (4, 1, 64): (117520, 84752), (4, 2, 32): (112016, 46480),
             (4, 2, 64): (158480, 92944), (4, 3, 64): (133904, 101136), (4, 4, 64): (121616, 109328),
             (8, 1, 64): (125712, 92944), (8, 2, 64): (105232, 109328), (8, 3, 64): (127760, 131856),
             (8, 4, 64): (144144, 148240), (8, 3, 32): (78224, 82320)}
    from miso_amd import _lib
    lib = _lib.load()

    def asked(C, L, H, scat):
        g = _lib.Grid()
        g.n_levels = L
        for a in range(3):
            g.bound_min[a], g.bound_max[a] = -1.0, 1.0
        for l in range(L):
            lv = g.level[l]
            lv.C, lv.X, lv.Y, lv.Z = C, 8, 8, 8
            lv.sC, lv.sX, lv.sY, lv.sZ = 1, C, C * 8, C * 64
            lv.data, lv.grad = None, 0x100000 * (l + 1)
        m = _lib.Mlp()
        m.n_linear, m.in_dim, m.hidden_dim, m.out_dim = 3, C * L, H, 1
        return lib.miso_sdf_train_lds_bytes(ctypes.byref(g), ctypes.byref(m), int(scat))

    for (C, L, H), want in table.items():
        for scat in (True, False):
            got = asked(C, L, H, scat)
            assert got == want[0 if scat else 1], (C, L, H, scat)
            assert 0 < got <= 160 * 1024, (C, L, H, scat)
    assert asked(8, 3, 48, True) == 0          # a shape outside the table
    # (round 6: the bf16x3 pack -- 18 432 dwords of matrix pieces + 196 of biases / output weights at 64 x 64 with F in 17..32)
    assert asked(8, 3, 64, False) == 4 * (18628 + 8 * 64 * 28)       # nothing scattered: the eight-wavefront form, 128.8 KB
    assert asked(8, 4, 64, True) == 4 * (18628 + 4 * (64 * 36 + 64 * 4 * 8))
    feats = [torch.zeros(1, 8, 4, 4, 4).contiguous(memory_format=torch.channels_last_3d)] * 3
    meta = ops.GridMeta((-1.0,) * 3, (1.0,) * 3, 0, 0)
    assert ops.sdf_train_supported(feats, meta, [feats[0], None, None]) and not ops.sdf_train_supported(feats, meta, [None] * 3)
    ncdhw = [torch.zeros(1, 8, 4, 4, 4)] * 3          # channel stride != 1: no fused kernel takes the layout
    assert not ops.sdf_train_supported(ncdhw, meta, [ncdhw[0], None, None])


def _environment_reads():
    """-> (names, sites, literal): the variables the library reads -- getenv("NAME") in miso_amd/csrc, os.environ in the
    package's Python -- with the number of read sites and of those whose name is a string literal."""
    import glob
    names, sites, literal = set(), 0, 0
    csrc = os.path.join(ROOT, "miso_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))):
        code = re.sub(r"//[^\n]*", "", open(path).read())
        sites += len(re.findall(r"\bgetenv\s*\(", code))
        found = re.findall(r"\bgetenv\s*\(\s*\"([A-Za-z0-9_]+)\"\s*\)", code)
        literal += len(found)
        names.update(found)
    # (every source of the library is a .hip or a .hpp; Python reads go through `os.`: importing the names is refused)
    for path in sorted(glob.glob(os.path.join(ROOT, "miso_amd", "**", "*.py"), recursive=True)):
        code = open(path).read()
        assert not re.search(r"from\s+os\s+import[^\n]*\b(environ|getenv|putenv)\b", code), path
        sites += len(re.findall(r"\bos\s*\.\s*(?:environ|getenv|putenv)\b", code))
        found = re.findall(r"\bos\.environ(?:\.get|\.setdefault|\.pop)?\s*[\(\[]\s*[\"']([A-Za-z0-9_]+)[\"']", code)
        literal += len(found)
        names.update(found)
    return names, sites, literal


def test_readme_lists_every_environment_variable_the_library_reads():
    """The table under "Environment variables" in README.md is closed: it names exactly the variables that miso_amd/csrc
    reads through getenv and the Python package through os.environ, and every such read names its variable literally,
    so that none can be added without a row that says what it is for."""
    names, sites, literal = _environment_reads()
    assert sites == literal, "an environment read whose variable is not a string literal"
    assert names >= {"MISO_HIP_LIB", "MISO_EXACT_F32", "MISO_PULL_MC"}      # (the scan still finds what is known to be there)
    readme = open(os.path.join(ROOT, "README.md")).read()
    section = readme.split("### Environment variables", 1)[1].split("\n#", 1)[0]
    rows = [ln.split("|")[1] for ln in section.splitlines() if ln.startswith("| `")]
    listed = [n for cell in rows for n in re.findall(r"`([A-Za-z0-9_]+)`", cell)]
    assert len(listed) == len(set(listed)), "a variable is listed twice"
    assert set(listed) == names, (sorted(names - set(listed)), sorted(set(listed) - names))
