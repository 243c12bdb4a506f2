"""Host side of the decoder weight-gradient entry points (include/miso_hip.h: miso_sdf_wgrad,
miso_sdf_wgrad_workspace_floats): declared, bound and exported; the workspace size per instantiated shape; argument
checks that return before anything touches a device; and GridNet.forward on host tensors, which stays on the torch route.
No GPU is needed."""
import ctypes as C
import os
import re

import pytest
import torch

from miso_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fused_shapes():
    text = open(os.path.join(ROOT, "miso_amd", "csrc", "sdf_fused.hpp")).read()
    body = re.search(r"#define MISO_FUSED_SHAPES\(X\)((?:.*\\\n)*.*)\n", text)[1]
    shapes = [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", body)]
    assert len(shapes) >= 11
    return shapes


def _grid(c, l, size=8):
    g = _lib.Grid()
    g.n_levels = l
    for a in range(3):
        g.bound_min[a], g.bound_max[a] = -1.0, 1.0
    for i in range(l):
        lv = g.level[i]
        lv.C, lv.X, lv.Y, lv.Z = c, size, size, size
        lv.sC, lv.sX, lv.sY, lv.sZ = 1, c, c * size, c * size * size      # channels-last
    return g


def _mlp(f, h, nh, out_dim=1):
    m = _lib.Mlp()
    m.in_dim, m.hidden_dim, m.out_dim, m.n_linear = f, h, out_dim, nh + 2
    return m


def test_entry_points_are_declared_bound_and_exported():
    for name in ("miso_sdf_wgrad", "miso_sdf_wgrad_workspace_floats"):
        assert name in _lib.SIGNATURES
        fn = getattr(_lib.load(), name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
    assert _lib.SIGNATURES["miso_sdf_wgrad_workspace_floats"][0] is C.c_int64
    assert [f for f, _ in _lib.MlpGrad._fields_] == ["weight", "bias"]


def test_workspace_size_per_shape():
    lib = _lib.load()
    for c, l, h, nh in _fused_shapes():
        g, m = _grid(c, l), _mlp(c * l, h, nh)
        block = h * c * l + nh * h * h + h + (nh + 1) * h + 1      # every dW_l and db_l
        one = lib.miso_sdf_wgrad_workspace_floats(C.byref(g), C.byref(m), 1)
        big = lib.miso_sdf_wgrad_workspace_floats(C.byref(g), C.byref(m), 1 << 22)
        assert one == block, (c, l, h, nh)
        assert big % block == 0 and block < big <= 2 * 1024 * 1024      # capped: a few MB of floats, whatever n
        assert lib.miso_sdf_wgrad_workspace_floats(C.byref(g), C.byref(m), 262144) == big      # (shape, n) alone
        assert lib.miso_sdf_wgrad_workspace_floats(C.byref(g), C.byref(m), 0) == 0
    g, m = _grid(8, 3), _mlp(24, 48, 1)
    assert lib.miso_sdf_wgrad_workspace_floats(C.byref(g), C.byref(m), 4096) == 0
    assert lib.miso_sdf_wgrad_workspace_floats(None, C.byref(m), 4096) == 0


def test_argument_checks_return_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    packed = C.c_void_p((C.addressof(buf) + 15) & ~15)      # never read: every call below is refused first
    grads = _lib.MlpGrad()
    for i in range(3):
        grads.weight[i] = packed.value
    g, m = _grid(8, 3), _mlp(24, 64, 1)

    def call(grid, mlp, pk=packed, n=0, gsdf=None, mask=None, flags=0, gr=grads, ws=None, ws_floats=0):
        return lib.miso_sdf_wgrad(grid, mlp, pk, None, n, gsdf, mask, None, flags, C.byref(gr) if gr else None, ws,
                                  ws_floats, None)

    assert call(None, C.byref(m)) == _lib.E_BADARG == 2001
    assert call(C.byref(g), None) == 2001
    assert call(C.byref(g), C.byref(m), pk=None) == 2001
    assert call(C.byref(g), C.byref(m), n=-1) == 2001
    assert call(C.byref(g), C.byref(m), n=64) == 2001                               # no mask, no grad_sdf
    assert call(C.byref(g), C.byref(m), flags=_lib.F_GRAD_SDF_SORTED) == 2001       # binned cotangent without a binned batch
    assert call(C.byref(g), C.byref(m), gr=None) == 2001
    assert call(C.byref(g), C.byref(_mlp(24, 48, 1))) == _lib.E_UNSUPPORTED == 2002   # H = 48 is not instantiated
    assert call(C.byref(g), C.byref(_mlp(24, 64, 1, out_dim=2))) == 2002
    assert call(C.byref(_grid(8, 2)), C.byref(m)) == 2002                           # in_dim != sum of C
    # a workspace that is too small (levels with data, so that the check is reached)
    for i in range(3):
        g.level[i].data = packed.value
    need = lib.miso_sdf_wgrad_workspace_floats(C.byref(g), C.byref(m), 64)
    assert need > 0
    assert call(C.byref(g), C.byref(m), n=64, gsdf=packed, mask=packed, ws=packed, ws_floats=need - 1) == 2001
    assert call(C.byref(g), C.byref(m), n=64, gsdf=packed, mask=packed, ws=None, ws_floats=need) == 2001


def test_gridnet_forward_on_host_tensors_stays_on_the_torch_route(monkeypatch):
    from miso_amd import ops
    from miso_amd.grid_opt.models.grid_net import GridNet
    cfg = {"name": "grid_net", "spatial_dim": 3,
           "decoder": {"type": "mlp", "hidden_dim": 64, "hidden_layers": 1, "out_dim": 1, "pos_invariant": True,
                       "fix": False, "pretrained_model": None},
           "grid": {"type": "regular", "feature_dim": 8, "init_stddev": 3e-2, "bound": [[-1.0, 1.0]] * 3,
                    "base_cell_size": 0.5, "per_level_scale": 2, "n_levels": 2},
           "pose": {"optimize": False, "num_poses": 1}}
    torch.manual_seed(0)
    net = GridNet(cfg, device="cpu")

    def refuse(*a, **k):
        raise AssertionError("the fused route was taken on host tensors")

    monkeypatch.setattr(ops, "sdf_fused", refuse)
    taken = []
    query = net.query_feature
    monkeypatch.setattr(net, "query_feature", lambda x: taken.append(1) or query(x))
    assert all(p.requires_grad for p in net.decoder.parameters())
    # the torch route is query_feature + utils.grid_decode; its encode is a HIP operator without a host form, which says so
    with pytest.raises(RuntimeError, match="HIP device only"):
        net(torch.rand(50, 3) * 1.8 - 0.9)
    assert taken == [1]
    assert net.decoder.decoder_pack() is None      # a trainable decoder stays off every other fused consumer
    assert net.decoder.decoder_pack(trainable=True) is net.decoder.decoder_pack(trainable=True)
