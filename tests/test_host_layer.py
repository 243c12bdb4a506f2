"""The Python layer between the C ABI and grid_opt: refusals are typed (ops.NotCovered, raised before any launch, by
every wrapper that takes a decoder), GridAtlas remembers a refused query per set of feature tensors, and the two Adam
drivers of MappingStep (adam=dict(...): host scalars; adam_device=: device scalars) share one argument block and take
the same steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pack(dims, seed=3):
    from miso_amd import ops
    g = torch.Generator().manual_seed(seed)
    ws = [(torch.randn(o, i, generator=g) * 0.3).to(DEV) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(torch.randn(o, generator=g) * 0.1).to(DEV) for o in dims[1:]]
    return ops.DecoderPack(ws, bs)


def _levels(C, sizes, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, C, s, s, s, generator=g) * 0.05).to(DEV).contiguous(memory_format=torch.channels_last_3d)
            for s in sizes]


def test_every_decoder_wrapper_refuses_an_uncovered_shape_with_not_covered():
    """A 12-48-48-1 decoder (48 is neither 32 nor 64) does not pack: each wrapper that hands a decoder to the library
    raises ops.NotCovered before it fills, uploads or launches anything -- the seven that used to check by hand and
    those that went on to ctypes with m = None.  A decoder that packs over a grid outside the kernel table is refused
    by the library itself, through _lib.check, with the same type."""
    from miso_amd import ops
    n = 64
    feats = _levels(4, (4,))
    meta = ops.GridMeta.from_bound([[-1.0, 1.0]] * 3)
    bad = _pack((4, 48, 48, 1))
    assert bad.get() == (None, None)
    f32 = dict(device=DEV, dtype=torch.float32)
    x = torch.rand(n, 3, **f32) * 2 - 1
    g1, aux, slots = torch.ones(n, 1, **f32), torch.zeros(n, 4, **f32), torch.zeros(ops._lib.LOSS_SLOTS, 2, **f32)
    mask = torch.zeros(64 * 8, device=DEV, dtype=torch.int32)
    grads = [torch.zeros_like(f) for f in feats]
    sb = ops.SortedBatch(n, DEV).sort(x, meta)
    poses = torch.cat((torch.eye(3, **f32).reshape(-1), torch.zeros(3, **f32))).reshape(1, 12)   # R = I, t = 0
    q = ops.AtlasQuery()
    lm = ops.LmTrackStep(n, DEV, _pack((12, 32, 32, 1)))
    adam = ops.TrackAdamWindow(n, DEV, _pack((12, 32, 32, 1)), 1e-3, 2)
    rest = (None,) * 10
    calls = {
        "sdf_fwd_raw": lambda: ops.sdf_fwd_raw(x, feats, meta, bad, True),
        "sdf_wgrad_raw": lambda: ops.sdf_wgrad_raw(x, feats, meta, bad, g1, mask),
        "sdf_mask_words": lambda: ops.sdf_mask_words(bad),
        "AtlasQuery.__call__": lambda: q([feats], [meta], poses, bad, x=x),
        "AtlasQuery._backward": lambda: q._backward([feats], [meta], poses, bad, x, g1.reshape(-1), True, False,
                                                    [[False]], False),
        "AtlasQuery.trace": lambda: q.trace([feats], [meta], poses, bad, x, x, min_dist=1e-3, max_dist=1.0, max_iters=4,
                                            epsilon=1e-4),
        "sdf_bwd_raw": lambda: ops.sdf_bwd_raw(x, feats, meta, bad, g1, mask, True, [True], grads),
        "sdf_bwd_rows_raw": lambda: ops.sdf_bwd_rows_raw(x, feats, meta, bad, g1, mask, True, [True], grads),
        "sdf_fwd_loss_raw": lambda: ops.sdf_fwd_loss_raw(feats, meta, bad, sb, aux, mask, g1, slots),
        "sdf_fwd_loss_unsorted_raw": lambda: ops.sdf_fwd_loss_unsorted_raw(x, feats, meta, bad, aux, mask, g1, slots),
        "sdf_train_raw": lambda: ops.sdf_train_raw(feats, meta, bad, sb, aux, slots, grads),
        "sdf_train_unsorted_raw": lambda: ops.sdf_train_unsorted_raw(x, feats, meta, bad, aux, slots, grads),
        "LmTrackStep.__call__": lambda: lm(feats, meta, bad, *rest, "L2", 0.1, 1e-3),
        "TrackAdamWindow.step": lambda: adam.step(feats, meta, bad, *rest, "L2", 1.0, 0.1),
    }
    assert len(calls) == 14
    for name, call in calls.items():
        with pytest.raises(ops.NotCovered) as e:
            call()
        assert e.value.code == ops._lib.E_UNSUPPORTED and isinstance(e.value, RuntimeError), name
        assert "not covered by the fused kernels" in str(e.value), name
    assert all(not g.any() for g in grads)
    # the library's own refusal: the decoder packs, (C, levels, hidden, layers) = (4, 3, 32, 1) is not in the table
    three = _levels(4, (4, 4, 4))
    packs = _pack((12, 32, 32, 1))
    assert packs.get()[0] is not None and not ops.sdf_fused_supported(three, meta, packs)
    with pytest.raises(ops.NotCovered) as e:
        ops.sdf_fwd_raw(x, three, meta, packs, False)
    assert e.value.what == "miso_sdf_fwd" and e.value.code == ops._lib.E_UNSUPPORTED
    assert str(e.value) == "miso_sdf_fwd failed: shape not covered by the fused kernels (code 2002)"
    torch.cuda.synchronize()


def test_atlas_remembers_a_refused_query_per_set_of_feature_tensors(monkeypatch):
    """Two submaps, one level of C=12 on a 4^3 lattice: 12 % 4 == 0 lets a feature-only query past _fused_eligible, and
    (12, 1, .) is in no kernel table, so the launch is refused.  The fallback to the per-submap loop is taken because of
    ops.NotCovered and nothing else, and the refusal is remembered until a feature tensor's storage is rebound."""
    import golden_cases as gc
    from miso_amd import _lib, ops
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    bound = [[0.0, 2.0]] * 3
    torch.manual_seed(7)
    atlas = GridAtlas(gc.model_cfg(bound, 0.5, 2.0, 1, 12, 64, init_stddev=0.1), device=DEV)
    for s in range(2):
        atlas.add_submap(torch.tensor(bound), torch.eye(3), torch.tensor([[1.0 * s], [0.0], [0.25 * s]]), num_poses=1)
        atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
    atlas.to(DEV)
    assert tuple(atlas.get_submap(0).features[0].feature.shape) == (1, 12, 4, 4, 4)
    x = (torch.rand(100, 3, generator=torch.Generator().manual_seed(9)) * 5.0 - 1.0).to(DEV)   # some outside both bounds
    with torch.enable_grad():
        loop = atlas.query_feature(x).detach()                         # autograd on: the loop
    lib = _lib.load()
    built, real, inject = [], lib.miso_atlas_plan_build, []

    def spy(*args):
        built.append(1)
        return inject.pop() if inject else real(*args)

    monkeypatch.setattr(lib, "miso_atlas_plan_build", spy)
    with torch.no_grad():
        assert atlas._fused_eligible(x, want_sdf=False) is not None    # the Python-side test lets the shape through
        assert torch.equal(atlas.query_feature(x), loop) and len(built) == 1
        assert atlas._fused_eligible(x, want_sdf=False) is None        # ... the launch did not: remembered
        assert torch.equal(atlas.query_feature(x), loop) and torch.equal(atlas.query_feature(x), loop)
        assert len(built) == 1
        f = atlas.get_submap(1).features[0].feature
        f.data = f.data.clone()                                        # new storage: asked again, once
        assert torch.equal(atlas.query_feature(x), loop) and len(built) == 2
        assert torch.equal(atlas.query_feature(x), loop) and len(built) == 2
        # any other failure of the same call is no reason to fall back
        f.data = f.data.clone()
        inject.append(_lib.E_BADARG)
        with pytest.raises(ops.MisoError) as e:
            atlas.query_feature(x)
        assert e.value.code == _lib.E_BADARG and not isinstance(e.value, ops.NotCovered) and len(built) == 3
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,sort", [(4096, False), (16384, True)])
def test_both_adam_drivers_of_the_mapping_step_take_the_same_steps(n, sort):
    """MappingStep(adam=dict(lr=...)) (host scalars, its own moments) and MappingStep(adam_device=, adam_state=) (the
    caller's moments, scalars from the device table) over the same two levels, three steps each: both step every level
    in ONE launch through the same argument block (MappingStep._adam_block) and end with the same parameters and
    moments.  Not bit for bit, on the parent commit no more than here, and no more between two runs of ONE driver:
    unbinned (n = 4096) the gradient is a sum of float atomics, binned (n = 16384) the order of the points inside a tile
    run depends on the sort's LDS atomics -- so the bound is that of
    test_stream_launches_and_graph_replays_give_the_same_step, 2e-6 of the largest entry (measured on both commits:
    at most 2.8e-7 of it).  Which chunks have ever moved (the `active` flags) is no sum: equal."""
    from miso_amd import ops
    from miso_amd.step import MappingStep
    from test_train_fused import _setup
    feats, meta, pack, x, aux = _setup(4, (8, 16), 64, n, seed=43)
    aux[7, 0] = 0.0
    out = {}
    for mode in ("host", "device"):
        fs = [f.clone() for f in feats]
        kw = dict(adam=dict(lr=1e-3))
        if mode == "device":
            state = [(torch.zeros_like(f), torch.zeros_like(f), ops.adam_active_flags(f)) for f in fs]
            kw = dict(adam_device=ops.AdamDeviceStep(1e-3, 0.9, 0.999, 1e-8, DEV), adam_state=state)
        st = MappingStep(fs, meta, pack, n, "L1", 1.0, 0.1, 0.15, keep_sdf=False, use_graph=False, sort=sort, **kw)
        assert (st.sorted is not None) == sort and not st._use_graph
        st.set_batch(x, aux[:, 0:1], aux[:, 1:2], aux[:, 2:3], aux[:, 3:4])
        for _ in range(3):
            st.run()
        torch.cuda.synchronize()
        blocks = st._adam_block()
        assert len(blocks) == 1 and len(blocks[0][0]) == 2              # one launch for both levels, in both drivers
        out[mode] = [t for f, s in zip(fs, st.adam_state) for t in (f, *s)]
    for k, (a, b) in enumerate(zip(out["host"], out["device"])):
        diff = (a.float() - b.float()).abs().max().item()
        print(f"n={n} sort={sort} level {k // 4} {('param', 'exp_avg', 'exp_avg_sq', 'active')[k % 4]}: "
              f"max |host - device| = {diff:.3e}, max |device| = {b.float().abs().max().item():.3e}")
        if k % 4 == 3:
            assert torch.equal(a, b)
        else:
            assert diff <= 2e-6 * b.abs().max().item()
