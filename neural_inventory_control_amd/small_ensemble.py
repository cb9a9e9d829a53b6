"""`SmallPolicyEnsemble`: K small policies of ONE architecture (`vanilla_one_store` / `vanilla_serial`, 32-wide MLPs) trained or
evaluated on ONE batch with one forward launch, one backward launch and one reduction for all of them
(`nic_small_rollout_ensemble_*`, csrc/small_rollout16.hip / small_rollout.hip / small_reduce.hip: grid y = model).

A wavefront of the whole-horizon kernels is one serial chain of T periods, and at the batch sizes these policies are trained
with (1,024 - 8,192 scenarios) most SIMDs have no wavefront: seeds, learning rates or initialisations of one architecture ride
in them instead of paying K steps.  Every model runs the instruction stream of the single-model kernels on its own slice of the
buffers, so its costs and gradients are the bits `FusedRollout.run` gives for that model alone (trainer.py:181-216 once per model).

`run` alone leaves the optimizer to the caller (K optimizers, or one with K parameter groups, step the models independently) and
packs all K models' weights again every call.  The whole training step is `train_step`: after `bind_parameters()` every model's
`weight` / `bias` are views of its row of `weights [K][P]` (the packed layout IS `nn.Linear`'s: per layer the weight, row-major,
then the bias), so nothing is packed, and an `EnsembleAdam` (ensemble_adam.py) updates all K rows with two launches - six
launches a step (forward, backward, two of the reduction, prepare, update) and no per-model Python.  `use_graph` replays them from
one captured sequence per batch shape (launch_replay.py); `fit` is the epoch loop over `train_step` with the best weights per
model kept on the device.

The K models need not share the batch: `run`, `train_step` and `fit` take a list (or tuple) of I batch dicts in place of one, I
dividing K, and model m then runs on instance m // (K // I) - its own demand trace, initial state and cost / lead-time tables
(`nic_small_rollout_instances_*`: the same launch pair, every model reading its instance's inputs).  That is the reference's
hyper-parameter grid over a setting (one_store_lost.yml: underage_cost 4, 9, 19, 39) x seeds in one engine.  The instances share B,
the trace length, the pipeline shape (lead times may differ within it) and the flags; `check_instances` names the first mismatch.
The engine owns the instance-stacked inputs per batch shape (demand [I][T_total][1][ldb], state0 [I][F][ldb], one stacked tensor
per table) at fixed addresses, so a replayed step stages and pins nothing.  A plain dict is the one-batch path.  Either kind of
input is only staged differently (`_stage_batch`, `_stage_instances`): from the descriptor on, `_step` is one path.

The packed-row layout, binding, the frames of `run` / `train_step`, `fit` and the generic model checks are `EnsembleStep`'s
(ensemble_step.py, shared with `HorizonPolicyEnsemble`), model and batch preparation are the functions every engine calls
(policy_layers.py, layout.py: no single-model engine is built here); this module has the small policies' rules, the batch
shapes' buffers and their launch replay, the staging and the launches.

Per-model early stopping: once `set_active(mask)` has been called (`fit(trainer_params=...)` does it), every launch of a step goes
through its `_active` entry point with the engine's `active [K]`: the workgroups of a model whose entry is zero return at entry, the
reduction and the optimizer skip its rows, so a stopped model costs no kernel time beyond its workgroups' dispatch and its weights,
moments and buffers keep their bits; its returned totals are NaN (and with `run(train=True)` its `param.grad` keep the last values
they had).  The grid is not shrunk to the active count.  A replayed capture holds the mask's address and reads its contents.

YAML / `main_run` wiring, a `torch.library` operator and multi-GPU sharding are not part of this engine.
"""
import torch

from . import small_rollout as sr
from .ensemble_step import (check_instances, check_model_list, EnsembleStep, grad_views, instance_replicas,
                            refresh_instance_tables, stack_instance_tables, table_layouts)
from .ensemble_step import pack_ensemble_weights  # noqa: F401  (a re-export)
from .launch_replay import LaunchReplay, ReplayedEngine
from .layout import demand_trace_soa, fill_initial_state, Table
from .policy_layers import HEADS, upper_bound
from .rollout import FusedRollout  # noqa: F401  (a re-export)

SMALL_POLICIES = ("vanilla_one_store", "vanilla_serial")


def _arch(m):
    a = m.nn_args
    return (a["name"], tuple(a["neurons_per_hidden_layer"]["master"]), a["output_sizes"]["master"])


def _hidden_rule(i, m):
    hidden = _arch(m)[1]
    if not (1 <= len(hidden) <= 3 and all(w == sr.H for w in hidden)):
        raise ValueError(f"model {i}: the whole-horizon kernels take 1..3 hidden layers of {sr.H} neurons, got {list(hidden)}")


def _upper_bound_rule(i, m, first):
    if _arch(m)[0] == "vanilla_serial" and upper_bound(m) != upper_bound(first):
        raise ValueError(f"model {i}: warehouse_upper_bound {upper_bound(m)} differs from model 0's {upper_bound(first)}")


def check_models(models):
    """The models an ensemble takes: K >= 1 policies `FusedRollout`'s small route takes, of one architecture - the same policy,
    layer sizes (1..3 hidden layers of 32, the same head) and `warehouse_upper_bound`.  ValueError names the first mismatch.
    Host-side only; the setting's side of `SmallRolloutPlan.supports` is checked when the first batch arrives."""
    return check_model_list(models, "SmallPolicyEnsemble", SMALL_POLICIES, f"the ELU MLP policies {SMALL_POLICIES}", _arch,
                            "architecture {} differs from model 0's {}", _hidden_rule, _upper_bound_rule)


class _ShapeState:
    """What ONE batch shape (the key of `_setup`) owns: the buffers sized for it and the launch-replay state whose captures hold
    their addresses, its staged demand trace and its pinned problem.  Weights, gradients and optimizer state depend on (K, P)
    only and are the engine's."""
    FIELDS = ("plan", "state0", "rewards", "final", "totals", "slices", "scratch", "strides", "ens", "states", "hidden", "logits", "slab",
              "g_reward", "g_reward_key",
              # I problem instances: the stacked inputs (demand [I][T_total][1][ldb], state0 [I][F][ldb], the problem whose tables are
              # [I][...]), the NicSmallInstances strides and the instances' problems the tables were last copied from
              "inst_demand", "inst_state0", "inst_prob", "inst", "inst_sources")

    def __init__(self, use_graph):
        for name in self.FIELDS:
            setattr(self, name, None)
        self.replay = LaunchReplay()
        self.replay.use_graph = use_graph


_MAX_KEPT_SHAPES = 4   # other batch shapes kept while their launches are replayed (an epoch has up to four: full / short x train / dev)


class SmallPolicyEnsemble(EnsembleStep, ReplayedEngine):
    def __init__(self, models, problem_params, device):
        super().__init__(check_models(models), problem_params, device)   # (`grad` here: [K][P rounded up to 4])
        self.head = HEADS[self.models[0].nn_args["name"]]
        self._ub_cache = {}             # `upper_bound`'s: model 0's bound is read from the device once, not per step
        self.small_lane_scenarios = 0   # 16 or 32 scenarios per wavefront (0: small_rollout.lane_width's rule)
        self._key = None
        self._shape = _ShapeState(False)   # the current batch shape's buffers and LaunchReplay (read as `ens.rewards`, `ens.plan`, ...)
        self._shapes = {}               # key -> _ShapeState of the other shapes whose launches are replayed

    def __getattr__(self, name):   # (only reached for names the engine itself does not have)
        if name in _ShapeState.FIELDS:
            return getattr(self._shape, name)
        raise AttributeError(name)

    # ---- launch mode: `use_graph` True / False / "auto" (launch_replay.py) is the engine's, the rest is per batch shape -----------------
    _replay = property(lambda self: self._shape.replay)

    @property
    def use_graph(self):
        return self._shape.replay.use_graph

    @use_graph.setter
    def use_graph(self, value):
        self._shape.replay.use_graph = value
        if value is False:
            self._shapes = {}   # (nothing is replayed any more: the other shapes' buffers and captures go)
        for st in self._shapes.values():
            st.replay.use_graph = value

    # ---- buffers: weights and gradients once per engine (ensemble_step.py), the rest once per (B, T, K) -------------------------------
    def _switch_shape(self, key):
        """Batch shape `key` becomes the current one.  The outgoing shape is kept while its launches are replayed (its captures
        hold its buffers' addresses; an epoch alternates between a few shapes), else its buffers are released before the new
        shape is sized."""
        old = self._shape
        if self._key is not None and old.replay.on():
            self._shapes[self._key] = old
        self._shape = self._shapes.pop(key, None) or _ShapeState(old.replay.use_graph)
        while len(self._shapes) > _MAX_KEPT_SHAPES:
            self._shapes.pop(next(iter(self._shapes)))
        self._key = key

    def _setup(self, prob, T, train, instances=()):
        """Sizes what this batch needs; returns the models' layers (None once the parameters are bound) and their sizes, for
        `_ready_weights`.  `instances`: what the key of a list-of-instances batch carries besides the shape (I, the trace length,
        the tables' layouts); a one-batch run has none."""
        K, dev, ld = self.n_models, self.device, prob.ldb
        z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        F = prob.S * prob.Ws + (0 if self.head == "softplus" else prob.Wn * prob.Ww + prob.E * prob.We)
        lins, dims = self._layers(F)
        if dims[0] != F or not sr.SmallRolloutPlan.supports(prob, self.head, dims):
            raise ValueError(f"SmallPolicyEnsemble: the whole-horizon kernels do not take this setting / policy (layer sizes {dims}, "
                             f"{F} state rows)")
        if not self._bound:   # (bound: sized when they were bound, and `dims` are theirs)
            self._model_buffers(dims)
        key = (prob.B, T, K, tuple(dims), prob.Ws, prob.Wn, prob.Ww, prob.E, prob.We) + tuple(instances)
        if self._key != key:
            self._switch_shape(key)
        sh = self._shape
        if sh.plan is None:
            sh.plan = plan = sr.SmallRolloutPlan(prob, self.head, dims)
            sh.state0 = z(F, ld)
            sh.rewards, sh.final = z(K, T, ld), z(K, F, ld)
            sh.totals = z(K, 2)
            # slice sizes: csrc/small_ensemble_plan.h through the library.  Histories and slab are sized for 16 scenarios per
            # wavefront (as FusedRollout sizes them: the 32-wide form uses the first F / n_out rows and half the slab rows)
            probe = plan.desc(T, 0, self.weights, sh.state0, sh.state0, 0.0, prob=prob, lane_scenarios=16)
            sh.slices = s = sr.ensemble_slices(probe)
            assert s["weights"] == self.weights.shape[1] and s["rewards"] == T * ld and s["final_state"] == F * ld
            sh.scratch = torch.empty(K, s["scratch"], device=dev)   # (a training step's need; the cost sums alone use less)
            sh.strides = dict(weights=s["weights"], rewards=s["rewards"], final_state=s["final_state"], scratch=s["scratch"])
            sh.ens = sr.ensemble_strides(K, **sh.strides)
        if train and sh.states is None:
            # the training buffers come with the first training run of a shape and stay: evaluation runs in between use the rest
            s = sh.slices
            sh.states, sh.hidden, sh.logits = z(K, s["states"]), z(K, s["hidden"]), z(K, s["logits"])
            sh.slab = z(K, s["slab_rows"], s["slab_row_stride"])
            sh.g_reward, sh.g_reward_key = z(ld), None
            if self.grad is None:   # (with the engine's first training run, and kept: it depends on (K, P) only)
                self.grad = z(K, s["grad"])
                self._grad_views = grad_views(self.grad, dims)
            sh.strides.update(states=s["states"], hidden=s["hidden"], logits=s["logits"], slab=s["slab"], grad=s["grad"])
            sh.ens = sr.ensemble_strides(K, **sh.strides)
        return lins, dims

    # ---- one batch, or one batch per instance -----------------------------------------------------------------------------------------
    def run(self, data, periods, ignore_periods=0, train=True, observation_params=None, demand_soa=None, grad_scale=None,
            accumulate_grads=False, discrete_allocation=False):
        """Rollout of one batch - or, `data` a list of I batches, of instance m // (K // I)'s batch - under every model (and, if
        `train`, d(mean loss)/d(theta) into every model's `param.grad`: views
        into one [K][P] gradient buffer, `accumulate_grads` adds - `small_rollout.assign_grads`).  Arguments as
        `FusedRollout.run`.  Returns (total [K], reported [K]) device tensors; `rewards` [K][T][ldb] holds the per-period costs."""
        return self._run((data, periods, ignore_periods, observation_params, demand_soa, grad_scale), train, accumulate_grads,
                         discrete_allocation)

    def train_step(self, data, periods, ignore_periods=0, optimizer=None, observation_params=None, demand_soa=None, grad_scale=None):
        """One whole training step of all K models (on one batch, or on a list of I instances' batches as in `run`): forward,
        backward, the reduction's two launches and `optimizer`'s two (an
        `EnsembleAdam` over this engine's (K, P)) - no packing, no `param.grad`, no per-model Python.  Needs `bind_parameters()`.
        Returns (total [K], reported [K]) of the step BEFORE the update, as `run` does."""
        return self._train_step((data, periods, ignore_periods, observation_params, demand_soa, grad_scale), optimizer)

    # ---- staging: what differs between the two kinds of input.  Each returns (the problem, demand trace and initial state the
    # descriptor points at), the NicSmallInstances or None, and what the input adds to the captures' variant and to their key --------------
    def _stage_batch(self, data, T, shift, train, demand_soa, optimizer):
        """One batch for all K models.  A captured sequence holds raw pointers: it reads the pinned problem's tables and the staged
        demand trace, refreshed in place."""
        prob = self._problem_for(data)
        if demand_soa is None:
            demand_soa = demand_trace_soa(data["demands"], prob.ldb, self.device)
        if demand_soa.shape[0] < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        self._ready_weights(*self._setup(prob, T, train), optimizer)
        sh = self._shape
        prob = sh.replay.pin_problem(prob)
        demand_soa = sh.replay.stage_demand(demand_soa)
        fill_initial_state(sh.state0, prob, data, stores_only=self.head == "softplus")
        return (prob, demand_soa, sh.state0), None, (), ()

    def _stage_instances(self, datas, T, shift, train, demand_soa, optimizer):
        """A list of I batches: model m runs on datas[m // (K // I)].  The instances' inputs are copied into this batch shape's
        stacked buffers (the tables only when the batches present other tensors than last time), whose addresses a captured
        sequence keeps: nothing is pinned or staged.  A caller's demand_soa is read in place, so its address is part of the
        capture's key."""
        dev, K, I = self.device, self.n_models, len(datas)
        instance_replicas(I, K, "SmallPolicyEnsemble")   # (before anything is built from the batches)
        probs = [self._problem_for(data) for data in datas]
        lengths = [int(data["demands"].shape[2]) for data in datas]
        check_instances(probs, K, lengths)
        prob0 = probs[0]
        B, ld, T_total = prob0.B, prob0.ldb, lengths[0]
        if T_total < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        if demand_soa is not None and tuple(demand_soa.shape) != (I, T_total, 1, ld):
            raise ValueError(f"SmallPolicyEnsemble: demand_soa of a list of instances must be [I][T_total][1][ldb] = {(I, T_total, 1, ld)}, "
                             f"got {tuple(demand_soa.shape)}")
        self._ready_weights(*self._setup(prob0, T, train, instances=("instances", I, T_total, table_layouts(prob0))), optimizer)
        sh = self._shape
        F = sh.plan.F
        if sh.inst_state0 is None:
            sh.inst_state0 = torch.zeros(I, F, ld, device=dev)
            sh.inst_prob, table_strides = stack_instance_tables(probs)
            sh.inst_sources = probs
            sh.inst = sr.instance_strides(I, state0=F * ld, demand=T_total * ld, **table_strides)
        else:   # (other batches than last time: their tables into the stacked ones, in place)
            sh.inst_sources = refresh_instance_tables(sh.inst_prob, sh.inst_sources, probs)
        if demand_soa is None:
            if sh.inst_demand is None:
                sh.inst_demand = torch.zeros(I, T_total, 1, ld, device=dev)
            demand_soa = sh.inst_demand
            for i, data in enumerate(datas):
                demand_soa[i, :, :, :B].copy_(data["demands"].permute(2, 1, 0))
        for i, data in enumerate(datas):
            fill_initial_state(sh.inst_state0[i], prob0, data, stores_only=self.head == "softplus")
        return (sh.inst_prob, demand_soa, sh.inst_state0), sh.inst, (I,), (I, demand_soa.data_ptr())

    def _step(self, data, periods, ignore_periods, observation_params, demand_soa, grad_scale, train, discrete_allocation, optimizer):
        """`data` a dict: all K models on one batch (`nic_small_rollout_ensemble_*`); a list or tuple of I dicts: model m on its
        instance's (`nic_small_rollout_instances_*`, also for I = 1).  The kind of input decides the staging, the launch pair's
        entry points and what it adds to the captures' variant and key; the rest is one path."""
        K, T = self.n_models, periods
        shift = observation_params["demand"]["period_shift"] if observation_params else 0
        stage = self._stage_instances if isinstance(data, (list, tuple)) else self._stage_batch
        (prob, demand_soa, state0), inst, variant, key = stage(data, T, shift, train, demand_soa, optimizer)
        sh, B, ld = self._shape, prob.B, prob.ldb
        replay = sh.replay
        ub = upper_bound(self.models[0], self._ub_cache) if self.head != "softplus" else 0.0
        width = sr.lane_width(self.small_lane_scenarios, train, B)
        desc = sh.plan.desc(T, shift, self.weights, demand_soa, state0, ub, round_orders=discrete_allocation, prob=prob,
                            lane_scenarios=width)
        hist = (sh.states, sh.hidden, sh.logits) if train else (None, None, None)
        n_el = T * ld
        if train:
            if grad_scale is None:
                grad_scale = 1.0 / (B * T * self.problem_params["n_stores"])
            sh.g_reward_key = sr.set_g_reward(sh.g_reward, B, grad_scale, sh.g_reward_key)
        if inst is None:
            fwd, bwd_wgrad, where = sr.small_rollout_ensemble_fwd, sr.small_rollout_ensemble_bwd_wgrad, (desc, sh.ens)
        else:
            fwd, bwd_wgrad, where = sr.small_rollout_instances_fwd, sr.small_rollout_instances_bwd_wgrad, (desc, sh.ens, inst)

        # once a mask has been set every launch goes through its `_active` entry point (None: the launches as they always were)
        mask = self._mask()
        masked = {} if mask is None else {"active": mask}

        def launches():
            fwd(*where, sh.rewards, sh.final, *hist, **masked)
            self._note("fwd")
            if train:
                row = sh.slab.shape[2]
                bwd_wgrad(*where, *hist, Table(sh.g_reward, 0, 1), sh.slab, row, **masked)
                self._note("bwd")
                sr.small_rollout_ensemble_reduce(sh.ens, sh.slab, sr.slab_rows_written(B, width), row, self.grad.shape[1], self.grad,
                                                 sh.rewards, n_el, ignore_periods * ld, sh.totals, sh.scratch, **masked)
            else:   # the same reduction, costs only: an evaluation pass returns the very bits a training pass does
                sr.small_rollout_ensemble_reduce(sh.ens, None, 0, 0, 0, None, sh.rewards, n_el, ignore_periods * ld, sh.totals,
                                                 sh.scratch, **masked)
            self._note("reduce")
            if optimizer is not None:
                optimizer.step(self.weights, self.grad, **masked)

        # what a captured sequence bakes in besides this shape's buffers.  Engine-wide things are the `variant` (a change drops this
        # shape's captures now, another shape's when it is current again); the optimizer's buffers, which only a training step's
        # sequence holds, are part of the capture's key, so evaluations in between (`fit`) change nothing
        if replay.on():
            replay.set_variant((K,) + variant + (self.small_lane_scenarios, self.weights.data_ptr(), ub,
                                                 None if mask is None else mask.data_ptr()))
        opt_key = optimizer and optimizer.capture_key()   # (clipping on or off is part of it: the two run other launches)
        replay.probe_begin(train)
        replay.call((train, opt_key, ignore_periods, shift, bool(discrete_allocation), width, mask is not None) + key, launches)
        replay.probe_end()
        replay.ran()
        # outside the capture: the caller's tensors must not change under a later step, and the rows of inactive models - which no
        # launch wrote, so they hold an earlier run's values - become NaN by the mask's contents now
        return self._mask_totals(sh.totals.clone())
