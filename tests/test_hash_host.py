"""Hash-indexed feature levels, everything that needs no GPU: the row index and its known answers, the module and the
config (grid.type 'hash'), the routes that refuse such a grid, include/miso_hash.h against the binding and against gcc,
and the refusals of its entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hash_cases as hc
import sampler_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "miso_hash.h")
E_BADARG = 2001


# --------------------------------------------------------------------------- #
# the index
# --------------------------------------------------------------------------- #
def test_hash_known_answers():
    for (i, j, k), log2, want in hc.KNOWN:
        dims = (2048, 2048, 2048)                      # 2^33 vertices: hashed at every log2 the table allows
        assert int(hc.row_index(i, j, k, dims, log2)) == want, ((i, j, k), log2)
    # products wrap in uint32: the same rows from Python integers reduced by hand
    for (i, j, k), log2, want in hc.KNOWN:
        h = (i ^ ((j * hc.PRIME_Y) & 0xFFFFFFFF) ^ ((k * hc.PRIME_Z) & 0xFFFFFFFF)) & ((1 << log2) - 1)
        assert h == want


def test_rows_dense_up_to_the_table_and_hashed_beyond():
    from miso_amd import _lib, ops
    lib = _lib.load()
    for dims, log2, rows, dense in (((16, 16, 16), 12, 4096, True),           # X Y Z == 2^B: dense-indexed
                                    ((17, 16, 16), 12, 4096, False),          # one more plane: hashed
                                    ((4097, 1, 1), 12, 4096, False),          # 2^B + 1 vertices
                                    ((4096, 1, 1), 12, 4096, True),
                                    ((5, 7, 3), 8, 105, True), ((5, 7, 3), 6, 64, False),
                                    ((2048, 2048, 2048), 19, 1 << 19, False),  # 2^33 vertices: no overflow of the count
                                    ((2048, 2048, 2048), 28, 1 << 28, False),
                                    ((2 ** 31 - 1,) * 3, 28, 1 << 28, False)):
        assert hc.level_rows(dims, log2) == (rows, dense), (dims, log2)
        assert ops.hash_level_rows(dims, log2) == (rows, dense)
        assert lib.miso_hash_rows(*dims, log2) == rows
    for dims, log2 in (((0, 4, 4), 12), ((4, 4, -1), 12), ((4, 4, 4), 3), ((4, 4, 4), 29)):
        assert lib.miso_hash_rows(*dims, log2) == 0
        with pytest.raises(ValueError):
            ops.hash_level_rows(dims, log2)
    # a dense-indexed level lists the dense grid's channels-last storage in order
    X, Y, Z = 5, 7, 3
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    assert np.array_equal(hc.row_index(i, j, k, (X, Y, Z), 8).reshape(-1), np.arange(X * Y * Z))
    t = torch.arange(X * Y * Z * 2, dtype=torch.float32).view(-1, 2)
    d = hc.dense_from_table(t, (X, Y, Z), 8)
    assert torch.equal(d.permute(0, 2, 3, 4, 1).reshape(-1, 2), t)


def test_rows_collide_in_the_equivalence_shapes():
    """What the GPU tests rely on: the 23 x 17 x 9 level is hashed at both table sizes with several vertices on EVERY
    row (52..59 at log2 6, 10..17 at log2 8); the 5 x 7 x 3 level is hashed with collisions at log2 6 and dense-indexed
    at log2 8."""
    def counts(dims, log2):
        X, Y, Z = dims
        k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        rows, dense = hc.level_rows(dims, log2)
        return np.bincount(hc.row_index(i, j, k, dims, log2).reshape(-1), minlength=rows), dense

    small, big = hc.DIMS
    for log2, lo, hi in ((6, 52, 59), (8, 10, 17)):
        c, dense = counts(big, log2)
        assert not dense and (c.min(), c.max()) == (lo, hi)
    c, dense = counts(small, 6)
    assert not dense and c.max() == 3 and c.sum() == 105
    c, dense = counts(small, 8)
    assert dense and (c.min(), c.max()) == (1, 1)


def test_fp32_corner_terms_reproduce_the_oracle():
    """hash_cases.corner_terms32 (the reference of the table-gradient test) against oracle.trilinear_first64: the same
    cells and in-range corners, and fp32 weights whose float64 sum of products is the oracle's value within the value
    bar -- on every point kind, for a hashed and a dense-indexed level."""
    for log2 in hc.LOG2S:
        ts, ds, pts, go, o = hc.case(log2, 2)
        foff = 0
        for t, dims in zip(ts, hc.DIMS):
            rows, inb, w = hc.corner_terms32(hc.index_coords(pts.x, dims), dims, log2)
            v = t.double().numpy()[rows]                                            # (N,8,C)
            val = (np.where(inb[:, :, None], v, 0.0) * w.astype(np.float64)[:, :, None]).sum(1)
            cols = slice(foff, foff + t.shape[1])
            sc.check("hash-terms", f"log2 {log2} level {dims}", torch.from_numpy(val), o.value[:, cols],
                     sc.value_bar_weight(o)[:, cols])
            # no corner in range <=> the oracle's yardstick is zero there
            assert np.array_equal(inb.any(1), (o.value_c[:, cols] > 0).any(1).numpy())
            foff += t.shape[1]


# --------------------------------------------------------------------------- #
# module and config
# --------------------------------------------------------------------------- #
BOUND = [[-1.0, 1.3], [-0.7, 0.9], [0.0, 2.1]]


def _cfg(grid_type="hash", log2=8, fdim=4, levels=2, cell=0.5):
    import golden_cases as gc
    cfg = gc.model_cfg(BOUND, cell, 2.0, levels, fdim, 64, num_poses=2, init_stddev=0.01)
    cfg["grid"]["type"] = grid_type
    if log2 is not None:
        cfg["grid"]["log2_hashmap_size"] = log2
    return cfg


def _net(**kw):
    from miso_amd.grid_opt.models.grid_net import GridNet
    return GridNet(_cfg(**kw), device="cpu")


def test_module_shapes_and_refusals():
    from miso_amd.grid_opt.models.grid_modules import FeatureGrid, HashFeatureGrid
    bound = torch.tensor([[-1.0, 1.3], [-0.7, 0.9], [0.0, 2.1]])
    dense = FeatureGrid(d=3, fdim=4, bound=bound, cell_size=0.1)
    Z, Y, X = dense.feature.shape[2:]
    for log2, rows in ((8, 256), (19, X * Y * Z)):
        g = HashFeatureGrid(d=3, fdim=4, bound=bound, cell_size=0.1, init_stddev=0.1, log2_hashmap_size=log2)
        assert g.dims == (X, Y, Z) and tuple(g.feature.shape) == (rows, 4) and g.feature.is_contiguous()
        assert g.dense_indexed == (log2 == 19) and g.rows == rows
        assert g.feature.abs().max() > 0 and float(g.norm().detach()) > 0
        g.zero_features()
        assert float(g.norm().detach()) == 0
        g.randn_features(0.5)
        assert g.feature.std() > 0.2
        assert g.num_params() == rows * 4
        with pytest.raises(ValueError, match="latent alignment needs regular levels"):
            g.vertex_positions()
        with pytest.raises(RuntimeError, match="HIP device only"):
            g.interpolate(torch.zeros(3, 3))
    init = torch.randn(256, 2)
    g = HashFeatureGrid(d=3, fdim=2, bound=bound, cell_size=0.1, initial_feature=init, log2_hashmap_size=8)
    assert torch.equal(g.feature.detach(), init)
    for log2 in (3, 29):
        with pytest.raises(ValueError, match="log2_hashmap_size"):
            HashFeatureGrid(d=3, fdim=4, bound=bound, cell_size=0.1, log2_hashmap_size=log2)
    for fdim in (3, 16):
        with pytest.raises(ValueError, match="channels"):
            HashFeatureGrid(d=3, fdim=fdim, bound=bound, cell_size=0.1, log2_hashmap_size=8)


def test_gridnet_hash_config_and_state_dict_round_trip():
    from miso_amd.grid_opt.models.grid_modules import HashFeatureGrid
    net = _net()
    assert net.grid_type == "hash" and len(net.features) == len(net.feature_stability) == 2
    for l, (f, s) in enumerate(zip(net.features, net.feature_stability)):
        assert isinstance(f, HashFeatureGrid) and isinstance(s, HashFeatureGrid)
        rows, dense = hc.level_rows(f.dims, 8)
        assert tuple(f.feature.shape) == (rows, 4) and tuple(s.feature.shape) == (rows, 1) and f.dims == s.dims
    assert net.features[0].dense_indexed and not net.features[1].dense_indexed          # 5 x 4 x 5 and 10 x 7 x 9
    assert _net(log2=None).features[0].log2_hashmap_size == 19                              # the default
    assert net._fused_decoder() is None
    other = _net()
    assert not torch.equal(other.features[1].feature, net.features[1].feature)
    other.load_state_dict(net.state_dict())
    for a, b in zip(other.features, net.features):
        assert torch.equal(a.feature, b.feature)
    with pytest.raises(RuntimeError):                                                      # a table of another size
        _net(log2=6).load_state_dict(net.state_dict())
    with pytest.raises(ValueError, match="grid type 'octree'"):
        _net(grid_type="octree")
    for log2 in (3, 29):
        with pytest.raises(ValueError, match="log2_hashmap_size"):
            _net(log2=log2)
    with pytest.raises(ValueError, match="channels"):
        _net(fdim=3)
    # sphere_trace declines on the host as well as through the decoder pack
    assert net.sphere_trace(torch.zeros(2, 3), torch.ones(2, 3)) is None


def test_routes_that_need_regular_levels_say_so():
    from miso_amd.grid_opt.models.encoder import Encoder
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    net = _net()
    with pytest.raises(ValueError, match="'hash'"):
        Encoder.register_grid_model(object.__new__(Encoder), net)
    atlas = GridAtlas(_cfg(), device="cpu")
    for _ in range(2):
        atlas.add_submap(torch.tensor(BOUND), torch.eye(3), torch.zeros(3, 1), num_poses=2)
        atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
    with pytest.raises(ValueError, match="latent alignment.*'hash'"):
        atlas.precompute_coordinates_for_alignment()
    from miso_amd.grid_opt.align.miso import pairwise_loss_latent
    with pytest.raises(ValueError, match="latent alignment.*'hash'"):
        pairwise_loss_latent(atlas, None, 0, 1, level=0)


def test_hash_encode_refuses_host_tensors_and_wrong_tables():
    from miso_amd import ops
    meta = ops.GridMeta.from_bound(sc.BOUNDS[hc.BOUND])
    ts = hc.tables(6, 4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.hash_encode(torch.zeros(5, 3), ts, meta, hc.DIMS, 6)
    for bad, dims, log2 in ((ts, hc.DIMS, 8),                                   # rows of another table size
                            ([ts[0]], hc.DIMS, 6),                              # a level short
                            ([t[:, :3] for t in ts], hc.DIMS, 6),               # 3 channels, and not contiguous
                            ([t.t().contiguous().t() for t in ts], hc.DIMS, 6)):
        with pytest.raises(ValueError):
            ops._fill_hash_grid(bad, meta, dims, log2)
    g = ops._fill_hash_grid(hc.tables(8, 4), meta, hc.DIMS, 8)
    assert [g.level[l].log2_rows for l in range(2)] == [0, 8] and [g.level[l].rows for l in range(2)] == [105, 256]


# --------------------------------------------------------------------------- #
# include/miso_hash.h
# --------------------------------------------------------------------------- #
def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_hash_header_parses_into_tables_of_its_own():
    from miso_amd import _lib
    names = sorted(set(re.findall(r"\b(miso_[a-z0-9_]+)\s*\(", _header_code())))
    assert names == sorted(_lib.HASH_SIGNATURES) == ["miso_hash_encode_bwd", "miso_hash_encode_fwd", "miso_hash_rows"]
    assert len(_lib.HASH_STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", _header_code())) == 2
    assert _lib.HASH_STRUCTS["miso_hash_level_t"] is _lib.HashLevel and _lib.HASH_STRUCTS["miso_hash_grid_t"] is _lib.HashGrid
    assert _lib.HASH_CONSTANTS == {"MISO_HASH_LOG2_MIN": 4, "MISO_HASH_LOG2_MAX": 28}
    # the tables of miso_hip.h hold nothing of it
    assert not set(_lib.HASH_SIGNATURES) & set(_lib.SIGNATURES) and not set(_lib.HASH_STRUCTS) & set(_lib.STRUCTS)
    hip = open(os.path.join(ROOT, "include", "miso_hip.h")).read()
    assert set(_lib.read_header(hip)[2]) == set(_lib.SIGNATURES)
    # on its own the header cannot be read (MISO_MAX_LEVELS is miso_hip.h's), and what the reader refuses there it refuses here
    text = open(HEADER).read()
    with pytest.raises(_lib.HeaderError):
        _lib.read_header(text)
    at = text.rindex("#ifdef __cplusplus")
    for extra in ("long miso_x(long);", "typedef struct { long a; } miso_x_t;", "#define MISO_X (1 << 3)", "#pragma pack(1)"):
        with pytest.raises(_lib.HeaderError):
            _lib.read_header(text[:at] + extra + "\n" + text[at:], base=(_lib.CONSTANTS, _lib.STRUCTS))


def test_hash_symbols_are_exported():
    from miso_amd import _lib
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in _lib.HASH_SIGNATURES:
        assert hasattr(raw, n), f"{n} declared in miso_hash.h but not exported"


def _gcc(tmp_path, name, text, *flags):
    src, out = tmp_path / name, tmp_path / (name + ".out")
    src.write_text(text)
    run = subprocess.run(["gcc", "-Werror", "-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(out)],
                         capture_output=True, text=True)
    return run, out


def test_hash_struct_layout_equals_the_header_as_gcc_sees_it(tmp_path):
    from miso_amd import _lib
    probes = []
    for n, c in _lib.HASH_STRUCTS.items():
        probes.append((f"sizeof({n})", ctypes.sizeof(c)))
        for f, _ in c._fields_:
            probes.append((f"offsetof({n}, {f})", getattr(c, f).offset))
            probes.append((f"sizeof((({n}*)0)->{f})", getattr(c, f).size))
    body = "".join(f'  printf("%zu\\n", {expr});\n' for expr, _ in probes)
    run, exe = _gcc(tmp_path, "layout.c", '#include <stdio.h>\n#include <stddef.h>\n#include "miso_hash.h"\n'
                    "int main(void) {\n" + body + "  return 0;\n}\n")
    assert run.returncode == 0, run.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    wrong = [(expr, g, want) for (expr, want), g in zip(probes, got) if g != want]
    assert len(got) == len(probes) and not wrong, wrong


_SIG_PRELUDE = """#include <type_traits>
#include "miso_hash.h"
template <class T> struct arg { using type = T; };
template <class T> struct arg<T*> {
  using U = std::remove_cv_t<T>;
  using type = std::conditional_t<std::is_class_v<U> || std::is_same_v<U, char>, U, void>*;
};
template <class F> struct abi;
template <class R, class... A> struct abi<R(A...)> { using type = typename arg<R>::type(typename arg<A>::type...); };
"""
_C_SCALARS = {"i": "int", "I": "unsigned int", "l": "long", "L": "unsigned long", "f": "float", "d": "double", "P": "void*"}


def test_hash_prototypes_equal_the_binding_as_a_cxx_compiler_sees_them(tmp_path):
    """Each declared function's type, reduced as tests/test_capi_symbols.py reduces miso_hip.h's (a scalar stays itself,
    a pointer to a miso struct keeps the struct, every other pointer is void*), against the type spelled from the
    binding's restype / argtypes; a binding with a narrowed argument must be refused."""
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

    sigs = _lib.HASH_SIGNATURES
    ok, err = accepted("sig.cpp", sigs)
    assert ok, err
    res, args = sigs["miso_hash_encode_fwd"]
    assert args[2] is ctypes.c_int64
    ok, err = accepted("narrow.cpp", {**sigs, "miso_hash_encode_fwd": (res, args[:2] + [ctypes.c_int32] + args[3:])})
    assert not ok and "static assertion failed" in err, err


# --------------------------------------------------------------------------- #
# refusals (host pointers: replayed on machines without a GPU only, as tests/test_capi_refusals.py is)
# --------------------------------------------------------------------------- #
def _hash_grid(dims=hc.DIMS, log2=6, C=4):
    from miso_amd import _lib
    keep = []
    g = _lib.HashGrid()
    g.n_levels = len(dims)
    for a in range(3):
        g.bound_min[a], g.bound_max[a] = -1.0, 1.0
    for l, d in enumerate(dims):
        rows, dense = hc.level_rows(d, log2)
        t = torch.zeros(rows, C)
        keep.append(t)
        lv = g.level[l]
        lv.table, lv.rows, lv.C = t.data_ptr(), rows, C
        lv.X, lv.Y, lv.Z = d
        lv.log2_rows = 0 if dense else log2
    return g, keep


@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="replayed on machines without a GPU only: the cases hand the library HOST pointers, and a "
                           "refusal that had regressed would launch a kernel on them -- never on a shared card")
def test_hash_entry_points_refuse_before_any_launch():
    from miso_amd import _lib
    lib = _lib.load()
    x, out = torch.zeros(4, 3), torch.zeros(4, 8)
    px, po = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def both(g, n=4, ld=8, xp=px, op=po):
        gp = None if g is None else ctypes.byref(g)
        return (lib.miso_hash_encode_fwd(gp, xp, n, op, ld, None), lib.miso_hash_encode_bwd(gp, xp, n, op, ld, None, None))

    assert both(None) == (E_BADARG, E_BADARG)                                   # NULL grid
    g, keep = _hash_grid()
    for n_levels in (0, 9):
        g.n_levels = n_levels
        assert both(g) == (E_BADARG, E_BADARG)
    for field, bad in (("C", 3), ("C", 0), ("C", 16), ("log2_rows", 3), ("log2_rows", 29), ("log2_rows", -1),
                       ("rows", 63), ("rows", 128), ("rows", 0), ("X", 0), ("Z", -1)):
        g, keep = _hash_grid()
        setattr(g.level[1], field, bad)
        assert both(g) == (E_BADARG, E_BADARG), (field, bad)
    g, keep = _hash_grid(log2=8)                  # level 0 is dense-indexed at log2 8 ...
    g.level[0].log2_rows = 8                      # ... so a hashed table of 256 rows is not this level's
    g.level[0].rows = 256
    assert both(g) == (E_BADARG, E_BADARG)
    g, keep = _hash_grid()
    g.level[0].log2_rows, g.level[0].rows = 0, 105      # hashed at log2 6, handed over as dense-indexed ... fits: accepted
    g.level[1].log2_rows, g.level[1].rows = 0, 64       # ... a dense-indexed level of 3519 vertices with 64 rows is not
    assert both(g) == (E_BADARG, E_BADARG)
    g, keep = _hash_grid()
    g.flags = 128
    assert both(g) == (E_BADARG, E_BADARG)               # a flag of the fused entries
    g, keep = _hash_grid()
    assert both(g, n=-1) == (E_BADARG, E_BADARG)
    assert both(g, ld=7) == (E_BADARG, E_BADARG)         # rows narrower than F = 8
    assert both(g, xp=None) == (E_BADARG, E_BADARG) and both(g, op=None) == (E_BADARG, E_BADARG)
    g.level[0].table = keep[0].data_ptr() + 4            # not 16-byte aligned
    assert both(g) == (E_BADARG, E_BADARG)
    g, keep = _hash_grid()
    g.level[1].table = None                              # the forward reads every table; a backward without grad_x does not
    assert lib.miso_hash_encode_fwd(ctypes.byref(g), px, 4, po, 8, None) == E_BADARG
    gx = torch.zeros(4, 3)
    assert lib.miso_hash_encode_bwd(ctypes.byref(g), px, 4, po, 8, ctypes.c_void_p(gx.data_ptr()), None) == E_BADARG
    # n == 0 with everything else in order is served without a launch
    g, keep = _hash_grid()
    assert both(g, n=0, xp=None, op=None) == (0, 0)
