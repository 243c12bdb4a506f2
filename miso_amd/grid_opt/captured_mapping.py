"""The trainer's captured mapping step: which (trainer, batch) pairs qualify, the checked step -- one MappingStep per
request followed by the usual optimizer.step() -- and the fast plan with the optimizer inside the replay.  Every rule
either of them decides by is written once here; Trainer.train_step (trainer.py) only calls in."""
import dataclasses
import logging
import weakref

import torch

from miso_amd import ops
from miso_amd.optim import DenseAdam, _KERNEL_MIN_NUMEL
from miso_amd.step import MappingStep
from .loss import MisoLossMapping, MisoLossMappingBase

logger = logging.getLogger(__name__)

def plain_mapping_loss(lf):
    """The loss is the plain mapping loss: nobody overrode MisoLossMappingBase.compute."""
    return isinstance(lf, MisoLossMappingBase) and type(lf).compute is MisoLossMappingBase.compute


def trained_levels(opt, feats):
    """Per level: does this optimizer train it.  (A level that requires grad but is not in the active optimizer -- the
    coordinate schedule trains one level at a time -- gets no gradient from a captured step.  Autograd would accumulate
    one that nothing consumes: the level's own optimizer starts with zero_grad() when its turn comes, reference
    trainer.py:206.  Parameters are the same either way.)"""
    held = {id(p) for group in opt.param_groups for p in group['params']}
    return tuple(id(f) in held and f.requires_grad for f in feats)


def adam_hyper(opt, mine):
    """The single (lr, betas, eps) of the parameter groups that hold the levels `mine`; None if they have several."""
    groups = [g for g in opt.param_groups if any(any(p is f for f in mine) for p in g['params'])]
    hyper = {(g['lr'], tuple(g['betas']), g['eps']) for g in groups}
    return next(iter(hyper)) if len(hyper) == 1 else None


def plain_dense_adam(opt):
    """A plain DenseAdam nobody listens to: the fast plan steps in place of optimizer.step(), which therefore must be
    DenseAdam's own and have no hooks waiting for it."""
    return type(opt) is DenseAdam and not opt._optimizer_step_pre_hooks and not opt._optimizer_step_post_hooks


def _other_params(opt, mine):
    return [p for g in opt.param_groups for p in g['params'] if not any(p is f for f in mine)]


def _leave_grads(others, feats, grads, need):
    """What the reference's optimizer.zero_grad(set_to_none=True) + backward (trainer.py:206) leave on the host.  Adam
    steps every parameter whose .grad is not None whatever its requires_grad, so a stale gradient on anything this step
    does not write (keyframe pose corrections left over from an adam tracking window, a locked level) must not
    survive."""
    for p in others:
        p.grad = None
    for f, g, nd in zip(feats, grads, need):
        if nd and f.grad is not g:
            f.grad = g


@dataclasses.dataclass(frozen=True)
class MappingRequest:
    """What one trainer step asks of a MappingStep, normalised once: the key of the step cache, and where both
    MappingStep constructions (checked step, fast plan) take their arguments from."""
    n: int
    padded: bool                # datasets with padded=True: the live row count stays on the device
    need: tuple                 # trained_levels()
    ignore: tuple
    loss_cfg: tuple             # (loss_type, weight_sdf, weight_fs, trunc_dist) as MappingStep takes them
    feat_ptrs: tuple
    # what the pointers stand for and the decoder that goes with them: carried along, not compared
    feats: list = dataclasses.field(compare=False, repr=False)
    pack: object = dataclasses.field(compare=False, repr=False)

    def new_step(self, meta, **how):
        return MappingStep([f.data for f in self.feats], meta, self.pack, self.n, *self.loss_cfg, need_levels=self.need,
                           keep_sdf=False, padded=self.padded, grads_cleared_by_optimizer=True, **how)


def mapping_request(trainer, model_input):
    """The request of this step, or None if the configuration does not qualify for a captured step: MisoLossMapping
    with only its sdf / free-space terms, a GridNet with a frozen MLP decoder, keyframe poses not optimised, dense Adam
    over feature grids."""
    lf, model, opt = trainer.loss_func, trainer.model, trainer.optimizer
    if not plain_mapping_loss(lf):
        return None
    if lf.loss_type not in ('L1', 'L2') or lf.weight_eik > 0 or lf.use_stability or lf.weight_clip > 0:
        return None
    # a subclass of DenseAdam will do here -- its own step() still runs; the fast plan wants plain_dense_adam()
    if not isinstance(opt, DenseAdam) or not hasattr(model, '_fused_decoder'):
        return None
    coords_frame = model_input['coords_frame'][0]
    if not coords_frame.is_cuda or coords_frame.shape[0] == 0:
        return None
    pack = model._fused_decoder()
    if pack is None or any(p.requires_grad for p in model.decoder.parameters()):
        return None
    if any(p.requires_grad for p in model.params_for_poses()):
        return None
    feats = [g.feature for g in model.features]
    need = trained_levels(opt, feats)
    if not any(need):
        return None
    loss_cfg = (lf.loss_type, float(lf.weight_sdf), float(lf.weight_fs) if lf.weight_fs > 0 else 0.0,
                0.0 if lf.trunc_dist is None else float(lf.trunc_dist))
    return MappingRequest(n=coords_frame.shape[0], padded=model_input.get('live_rows') is not None, need=need,
                          ignore=tuple(bool(v) for v in model.ignore_level_), loss_cfg=loss_cfg,
                          feat_ptrs=tuple(f.data_ptr() for f in feats), feats=feats, pack=pack)


def kept_plans(model):
    """The fast plans kept with this model.  The SLAM loop builds a new trainer (new optimizers) for every
    Mapper.mapping call, a few iterations each -- a later trainer over the same grids adopts a plan
    (_FastMappingPlan.adopt) instead of paying for a new step, a new capture and a new plan every time."""
    return model.__dict__.setdefault('_fast_plans', [])


def forget_plans(model):
    """Let go of the plans kept with this model, and with them their gradient, Adam and binning buffers."""
    model.__dict__.pop('_fast_plans', None)


class _FastMappingPlan:
    """The captured mapping step with the optimizer INSIDE the replay, and a host side reduced to what cannot be
    captured: one launch that writes the batch into the step's static buffers (keyframe lookup + frame -> world map +
    label rows: ops.mapping_batch), one graph replay (sort, forward + loss, backward, gradient, loss sum, Adam step
    count, Adam per level), the NaN-guard bookkeeping of DenseAdam.  Built by captured_mapping_step once a batch shape
    has come back; every call re-checks a fingerprint of everything the capture baked in (which tensors, which flags,
    which hyper-parameters) and hands the step back to the checked path if any of it moved.
    Why: at the Newer College shape (6 144 samples, 145 M grid floats) the GPU needs ~0.1 ms per step and the host
    side of the checked path 0.22 ms.  From MappingStep.STREAM_MIN_POINTS samples the same launches go to the stream
    one by one instead (host 105 instead of 85 us per step, the device 284 instead of 293 us at cfg-2 and 342 instead
    of 357 us at the ScanNet shape: no idle time between replays)."""

    @staticmethod
    def eligible_loss(lf, model):
        """ops.mapping_batch stands in for the loss's own frame -> world map: it must be the stock one."""
        return (type(lf).world_coords is MisoLossMapping.world_coords
                and type(lf).query_kf_pose is MisoLossMapping.query_kf_pose
                and hasattr(model, 'kf_key_index_table') and hasattr(model, 'updated_kf_poses_all'))

    @classmethod
    def build(cls, trainer, req, prev_step):
        opt, lf, model = trainer.optimizer, trainer.loss_func, trainer.model
        try:
            if not plain_dense_adam(opt) or not cls.eligible_loss(lf, model):
                return None
            mine = [f for f, nd in zip(req.feats, req.need) if nd]
            hyper = adam_hyper(opt, mine)
            if hyper is None:
                return None
            lr, (b1, b2), eps = hyper
            states = []
            for f in mine:
                st = opt.state.get(f)
                if (not st or 'active' not in st or f.numel() < _KERNEL_MIN_NUMEL or not f.is_cuda
                        or st['exp_avg'].stride() != f.stride() or st['exp_avg_sq'].stride() != f.stride()):
                    return None
                states.append(st)
            opt.resolve_guard()
            if len({st['step'] for st in states}) != 1:
                return None
            dev = ops.AdamDeviceStep(lr, b1, b2, eps, req.feats[0].device, count=states[0]['step'])
            bufs = iter([(st['exp_avg'], st['exp_avg_sq'], st['active']) for st in states])
            # use_graph=None: a replay below MappingStep.STREAM_MIN_POINTS, stream launches from there
            step = req.new_step(prev_step.meta, use_graph=None, sort=prev_step.sorted is not None,
                                share_grads=prev_step.grads, adam_device=dev,
                                adam_state=[next(bufs) if nd else None for nd in req.need])
        # what the two constructors raise on purpose: ops.NotCovered -- MappingStep, a (grid, decoder) shape outside the
        # fused kernels -- and ValueError -- AdamDeviceStep, betas whose step-scalar table would not end; _fill_grid, more
        # levels than the library takes.  Their asserts guard arguments this function forms itself: none is caught.
        except (ops.NotCovered, ValueError) as exc:
            logger.info(f"fast captured step not built ({type(exc).__name__}: {exc})")
            return None
        self = cls()
        self.step, self.dev, self.mine, self.hyper = step, dev, mine, hyper
        self.feats, self.need, self.pack, self.n, self.padded = list(req.feats), req.need, req.pack, req.n, req.padded
        self.dec_params = list(model.decoder.parameters())
        self.bind(trainer, states)
        plans = kept_plans(model)
        plans.append(self)
        del plans[:-8]
        return self

    def bind(self, trainer, states):
        opt = trainer.optimizer
        self.states = states
        self.opt_ref = weakref.ref(opt)
        self.other_params = _other_params(opt, self.mine)
        self.baked, self.owner = self.signature(trainer, states)

    @classmethod
    def adopt(cls, trainer, n, padded):
        """A plan built by an earlier trainer of the same model that fits this trainer's (fresh) optimizer: same grids,
        same levels to train, same loss and Adam hyper-parameters.  The optimizer's state for those levels becomes the
        plan's buffers, zeroed -- what a new torch.optim.Adam starts from."""
        opt, lf, model = trainer.optimizer, trainer.loss_func, trainer.model
        plans = kept_plans(model)
        if not plans or not plain_dense_adam(opt) or not plain_mapping_loss(lf):
            return None
        for plan in reversed(plans):
            if plan.n != n or plan.padded != padded:
                continue
            old = plan.opt_ref()
            if trained_levels(opt, plan.feats) != plan.need or adam_hyper(opt, plan.mine) != plan.hyper:
                continue
            # everything else the capture baked in must still hold (loss scalars, flags, decoder weights ...); the owner's
            # part of the signature is what changes hands below.  Asked before the optimizer's state is touched: a plan
            # that is refused leaves no trace in it, and an older plan that does fit still finds the optimizer fresh
            baked, _ = plan.signature(trainer, plan.states)
            if baked != plan.baked:
                continue
            states = [opt.state[f] for f in plan.mine]
            fresh = all(not st for st in states)
            if not fresh and old is not opt:
                continue                              # an optimizer with a history of its own: not ours to replace
            bufs = [a for a in plan.step.adam_state if a is not None]
            if not fresh and any(st.get('exp_avg') is not b[0] or st.get('exp_avg_sq') is not b[1] or st.get('active') is not b[2]
                                 for st, b in zip(states, bufs)):
                continue                              # its state no longer lives in the plan's buffers (a loaded state dict)
            if fresh and old is not None and old is not opt:
                # the optimizer that used the plan last is still alive (a trainer kept around, or one whose collection
                # is pending): it keeps its history in tensors of its own, the plan's buffers go to the new owner
                for st in plan.states:
                    for key in ('exp_avg', 'exp_avg_sq', 'active'):
                        if key in st:
                            st[key] = st[key].clone()
            if fresh:
                for st, (m, v, act) in zip(states, bufs):
                    m.zero_(); v.zero_(); act.zero_()
                    st.update(step=0, exp_avg=m, exp_avg_sq=v, active=act)
                plan.dev.set_count(0)
            plan.bind(trainer, states)
            # the plan's step ADDS to some levels and relies on its own Adam launch having left them zero.  The buffers
            # are shared with the checked-path steps of the trainers in between (share_grads), and a binned checked
            # step (optimizer.step(clear_grads=False)) leaves them non-zero: clear them here, once per adoption (64 MB
            # at the ScanNet shape, ~10 us), so the first replay does not add onto a stale gradient.
            plan.step.clear_added_levels()
            return plan
        return None

    def signature(self, trainer, states):
        """-> (baked, owner), cheap to read and compared before every replay.  baked: everything the capture baked in;
        a plan changes hands (adopt) only if this part still holds.  owner: what belongs to whoever runs the plan now --
        the optimizer's identity, its state addresses and its hook counts."""
        opt, lf, model = trainer.optimizer, trainer.loss_func, trainer.model
        return ((id(lf), id(model), lf.loss_type, float(lf.weight_sdf), float(lf.weight_fs), lf.trunc_dist,
                 lf.weight_eik > 0, bool(lf.use_stability), lf.weight_clip > 0,
                 tuple(bool(v) for v in model.ignore_level_),
                 tuple((f.data_ptr(), f.requires_grad) for f in self.feats),
                 tuple(p.requires_grad for p in self.dec_params),
                 tuple(p.requires_grad for p in model.params_for_poses()),
                 tuple((w.data_ptr(), w._version) for w in self.pack.weights),
                 tuple((g['lr'], tuple(g['betas']), g['eps'], len(g['params'])) for g in opt.param_groups)),
                (id(opt),
                 tuple((st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), st['active'].data_ptr()) for st in states),
                 len(opt._optimizer_step_pre_hooks), len(opt._optimizer_step_post_hooks)))

    def run(self, trainer, model_input, gt, sanitize=False):
        opt, model, step = trainer.optimizer, trainer.model, self.step
        coords_frame = model_input['coords_frame'][0]
        live = model_input.get('live_rows')
        if (coords_frame.shape[0] != self.n or not coords_frame.is_cuda or (live is not None) != self.padded
                or not plain_mapping_loss(trainer.loss_func)):
            return None
        baked, owner = self.signature(trainer, self.states)
        if baked != self.baked or owner != self.owner:
            return None
        # NaN guards of earlier steps that have arrived (a skipped step: the host counts go back, the device count never
        # moved); nothing here waits for the GPU
        self.dev.count -= opt.resolve_guard(block=False)
        count = self.states[0]['step']
        if any(st['step'] != count for st in self.states):
            return None
        if count != self.dev.count:
            self.dev.set_count(count)                         # a skipped step, a loaded state
        try:
            R_all, t_all = model.updated_kf_poses_all()
            with torch.no_grad():
                ops.mapping_batch(R_all, t_all.reshape(-1, 3), model.kf_key_index_table('KF'),
                                  model_input['sample_frame_ids'][0], coords_frame, gt['sdf'][0], gt['sdf_valid'][0],
                                  gt['sdf_signs'][0], model_input['weights'][0], step.x, step.aux, sanitize=sanitize)
        except (ValueError, AssertionError):
            return None                                       # a batch layout the launch does not take
        if live is not None:
            step.live_rows.copy_(live.reshape(1))
        step.run()
        # ---- what optimizer.step() does on the host ----------------------------------------------------------------
        _leave_grads(self.other_params, self.feats, step.grads, self.need)
        for f in self.mine:
            torch.autograd.graph.increment_version(f)         # written through raw pointers
        for st in self.states:
            st['step'] = count + 1
        self.dev.count = count + 1
        if hasattr(opt, '_step_count'):
            opt._step_count += 1
        if step._use_graph:
            total = step.total.clone()                        # a replay writes the address the capture baked in
        else:
            # stream launches take the pointer per launch: hand this step's scalar out and give the next step a new one --
            # no copy kernel on the launch stream (4 us per step)
            total, step.total = step.total, torch.empty_like(step.total)
        # guards resolved while making room: those steps were skipped on the device, whose counter never moved
        self.dev.count -= opt.note_guarded_step(total, self.states, host=step.host_total)
        return total


def captured_mapping_step(trainer, model_input, gt):
    """The common mapping configuration (mapping_request) as ONE graph replay (miso_amd.step.MappingStep: sort,
    forward + loss, backward, pull) followed by the usual optimizer.step().  Same arithmetic as the op-by-op path of
    Trainer.train_step; what goes away is ~60 launches and the autograd bookkeeping per iteration, which cost several
    times the 0.2 ms the GPU needs.  Returns the total loss, or None if the configuration does not qualify (the
    op-by-op path then runs)."""
    lf, model, opt = trainer.loss_func, trainer.model, trainer.optimizer
    fast = trainer._fast_plan
    if fast is not None:
        total = fast.run(trainer, model_input, gt)
        if total is not None:
            return total
        trainer._fast_plan = None         # something changed (e.g. the coordinate schedule moved to another optimizer)
    want_fast = trainer.cfg.get('fast_captured_step', True)
    if want_fast and kept_plans(model) and trainer._adopt_failed != id(opt):
        # a plan an earlier trainer of this model left behind (Mapper.mapping builds a trainer per call)
        cf = model_input['coords_frame'][0]
        fast = _FastMappingPlan.adopt(trainer, cf.shape[0], model_input.get('live_rows') is not None)
        if fast is not None:
            total = fast.run(trainer, model_input, gt)
            if total is not None:
                trainer._fast_plan = fast
                return total
        trainer._adopt_failed = id(opt)   # until the optimizer changes
    req = mapping_request(trainer, model_input)
    if req is None:
        return None
    cache = trainer._mapping_steps
    step = cache.get(req)
    if step is None:
        # a new request.  Datasets with a data-dependent row count (PosedSdfRgbd(padded=False): depth holes) change
        # n almost every batch: building a step and capturing a graph that is never replayed would cost more
        # than the op-by-op path.  So the step of a new request runs its launches eagerly and shares the gradient
        # buffers of the previous one; the graph is captured only when the same request comes back next time.
        prev = next(iter(cache.values()), None)
        cache.clear()            # one live step: batch sizes rarely alternate
        trainer._seen_again = False
        step = cache[req] = req.new_step(
            model.features[0].grid_meta(model.ignore_level_), use_graph=False,
            crowded=bool(trainer.cfg.get('crowded_batches', False)),
            share_grads=None if prev is None or prev.need_levels != list(req.need) else prev.grads)
    elif not step._use_graph and not trainer._seen_again:
        trainer._seen_again = True
        # same batch shape twice in a row: from now on one graph replay per step (small batches; large ones stay
        # on the stream, MappingStep.STREAM_MIN_POINTS)
        step.graph_by_size()
        if want_fast:
            # ... and from the step after this one, with the optimizer inside the replay (_FastMappingPlan)
            trainer._fast_plan_due = req
    with torch.no_grad():
        coords_frame = model_input['coords_frame'][0]
        frame_ids = model_input['sample_frame_ids'][0, :, 0]
        coords_world = lf.world_coords(model, coords_frame, frame_ids)
        step.set_batch(coords_world, gt['sdf'][0], gt['sdf_valid'][0], gt['sdf_signs'][0],
                       model_input['weights'][0], live_rows=model_input.get('live_rows'))
    step.run()
    mine = [f for f, nd in zip(req.feats, req.need) if nd]
    idle = [f for f, nd in zip(req.feats, req.need) if not nd]
    _leave_grads(_other_params(opt, mine) + idle, req.feats, step.grads, req.need)
    total = step.loss.sum()
    # small batches scatter into the step's persistent gradient buffers: the optimizer clears what it
    # consumed in the same pass (a memset of a 0.5 GB level costs as much as the rest of the step)
    clear = step.sorted is None
    # NaN guard (reference :213-219) on the device: the optimizer's kernels leave everything alone if the
    # loss is NaN and the host hears about it one step later -- no read-back between backward and step.
    # The step's scatter kernels flagged the 64-float chunks they wrote: Adam reads the flags, not the gradient
    opt.step(clear_grads=clear, guard=total,
             touched={id(f): t for f, t, nd in zip(req.feats, step.touched, req.need) if nd})
    due, trainer._fast_plan_due = trainer._fast_plan_due, None
    if due == req:
        trainer._fast_plan = _FastMappingPlan.build(trainer, req, step)
    return total
