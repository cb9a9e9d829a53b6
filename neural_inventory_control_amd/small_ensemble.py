"""`SmallPolicyEnsemble`: K small policies of ONE architecture (`vanilla_one_store` / `vanilla_serial`, 32-wide MLPs) trained or
evaluated on ONE batch with one forward launch, one backward launch and one reduction for all of them
(`nic_small_rollout_ensemble_*`, csrc/small_rollout16.hip / small_rollout.hip / small_reduce.hip: grid y = model).

A wavefront of the whole-horizon kernels is one serial chain of T periods, and at the batch sizes these policies are trained
with (1,024 - 8,192 scenarios) most SIMDs have no wavefront: seeds, learning rates or initialisations of one architecture ride
in them instead of paying K steps.  Every model runs the instruction stream of the single-model kernels on its own slice of the
buffers, so its costs and gradients are the bits `FusedRollout(model).run` gives for it (trainer.py:181-216 once per model).

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
per table) at fixed addresses, so a replayed step stages and pins nothing.  A plain dict is the one-batch path, unchanged.

YAML / `main_run` wiring, a `torch.library` operator and multi-GPU sharding are not part of this engine.
"""
import copy

import torch

from . import _lib
from . import small_rollout as sr
from .ensemble_step import bind_rows, EnsembleStep, materialized_width
from .launch_replay import LaunchReplay, ReplayedEngine
from .layout import demand_trace_soa, EnvProblem, Table
from .rollout import _HEADS, FusedRollout

SMALL_POLICIES = ("vanilla_one_store", "vanilla_serial")


def _upper_bound(model):
    ub = model.warehouse_upper_bound
    return float(ub.reshape(-1)[0]) if torch.is_tensor(ub) else float(ub)


def check_models(models):
    """The models an ensemble takes: K >= 1 policies `FusedRollout`'s small route takes, of one architecture - the same policy,
    layer sizes (1..3 hidden layers of 32, the same head) and `warehouse_upper_bound`.  ValueError names the first mismatch.
    Host-side only; the setting's side of `SmallRolloutPlan.supports` is checked when the first batch arrives."""
    models = list(models)
    if len(models) < 1:
        raise ValueError("SmallPolicyEnsemble needs at least one model")
    if len(models) > 65535:
        raise ValueError("SmallPolicyEnsemble takes at most 65,535 models")

    def arch(m):
        a = m.nn_args
        return (a["name"], tuple(a["neurons_per_hidden_layer"]["master"]), a["output_sizes"]["master"])
    for i, m in enumerate(models):
        name = getattr(m, "nn_args", {}).get("name") if hasattr(m, "nn_args") else None
        if name not in SMALL_POLICIES or not FusedRollout.supports(m):
            raise ValueError(f"model {i}: SmallPolicyEnsemble handles the ELU MLP policies {SMALL_POLICIES}, got {name!r}")
        hidden = arch(m)[1]
        if not (1 <= len(hidden) <= 3 and all(w == sr.H for w in hidden)):
            raise ValueError(f"model {i}: the whole-horizon kernels take 1..3 hidden layers of {sr.H} neurons, got {list(hidden)}")
        if any(lin.bias is None for lin in m.master_linears()):
            raise ValueError(f"model {i}: a layer without bias")
        if arch(m) != arch(models[0]):
            raise ValueError(f"model {i}: architecture {arch(m)} differs from model 0's {arch(models[0])}")
        if name == "vanilla_serial" and _upper_bound(m) != _upper_bound(models[0]):
            raise ValueError(f"model {i}: warehouse_upper_bound {_upper_bound(m)} differs from model 0's {_upper_bound(models[0])}")
    return models


def check_instances(probs, n_models, trace_lengths=None):
    """The problem instances one launch pair takes: I >= 1 `EnvProblem`s, I dividing the K models, that agree in everything the
    kernels take once - B, the pipeline shape, the flags, the trace length (`trace_lengths`, one per instance, if given) and every
    table's layout (present or not, uniform or per-scenario: one descriptor addresses all instances).  ValueError names the first
    mismatch.  Host-side only.  Returns the replicas per instance."""
    probs = list(probs)
    I = len(probs)
    if I < 1:
        raise ValueError("SmallPolicyEnsemble needs at least one problem instance")
    if n_models % I != 0:
        raise ValueError(f"SmallPolicyEnsemble: {I} problem instances do not divide {n_models} models")
    first = probs[0]
    for i, p in enumerate(probs[1:], 1):
        if p.B != first.B:
            raise ValueError(f"instance {i}: {p.B} scenarios, instance 0 has {first.B}")
        if trace_lengths is not None and trace_lengths[i] != trace_lengths[0]:
            raise ValueError(f"instance {i}: a demand trace of {trace_lengths[i]} periods, instance 0's has {trace_lengths[0]}")
        shape = lambda q: (q.S, q.Wn, q.E, q.Ws, q.Ww, q.We)  # noqa: E731
        if shape(p) != shape(first):
            raise ValueError(f"instance {i}: pipeline shape (S, Wn, E, Ws, Ww, We) = {shape(p)} differs from instance 0's {shape(first)}")
        if (p.lost_demand, p.maximize_profit) != (first.lost_demand, first.maximize_profit):
            raise ValueError(f"instance {i}: lost_demand / maximize_profit differ from instance 0's")
        for name in EnvProblem._TABLES:
            a, b = getattr(first, name), getattr(p, name)
            if (a.tensor is None) != (b.tensor is None):
                raise ValueError(f"instance {i}: table {name!r} is {'missing' if b.tensor is None else 'present'}, instance 0's is not")
            if a.tensor is not None and (a.scn_stride == 0) != (b.scn_stride == 0):
                kind = lambda t: "uniform" if t.scn_stride == 0 else "per-scenario"  # noqa: E731
                raise ValueError(f"instance {i}: table {name!r} is {kind(b)}, instance 0's is {kind(a)}")
            if a.tensor is not None and ((tuple(a.tensor.shape), a.loc_stride, a.sup_stride)
                                         != (tuple(b.tensor.shape), b.loc_stride, b.sup_stride)):
                raise ValueError(f"instance {i}: table {name!r} has shape {tuple(b.tensor.shape)}, instance 0's {tuple(a.tensor.shape)}")
    return n_models // I


def stack_instance_tables(probs):
    """An `EnvProblem` like probs[0] whose tables are [I][...] stacks of the instances' (instance 0 first: a descriptor built from it
    points at instance 0, instance i's copy of a table starts i x the returned stride behind) and {table: stride in floats}."""
    stacked, strides = copy.copy(probs[0]), {}
    for name in EnvProblem._TABLES:
        t = getattr(probs[0], name)
        if t.tensor is None:
            continue
        tensor = torch.stack([getattr(p, name).tensor.contiguous() for p in probs])
        setattr(stacked, name, Table(tensor, t.loc_stride, t.scn_stride, t.sup_stride))
        strides[name] = tensor[0].numel()
    return stacked, strides


def pack_ensemble_weights(linears_per_model, out=None):
    """[K][P]: row m = `pack_weights` of model m's layers, all K models in ONE torch.cat (one launch)."""
    K = len(linears_per_model)
    flat = sr.pack_weights([lin for lins in linears_per_model for lin in lins], None if out is None else out.view(-1))
    if flat.numel() % K != 0:
        raise ValueError("pack_ensemble_weights: the models do not have the same number of parameters")
    return flat.view(K, -1) if out is None else out


def grad_views(grad, F, n_hidden, n_out):
    """[(weight gradients per layer, bias gradients per layer)] per model: views into grad [K][>= P] in the packed-weight layout."""
    sl = sr.layer_slices(F, n_hidden, n_out)
    return [([grad[m, o:o + n * k].view(n, k) for o, n, k, _ in sl], [grad[m, bo:bo + n] for _, n, _, bo in sl])
            for m in range(grad.shape[0])]


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
        self.models = check_models(models)
        _lib.require_device()
        self.problem_params = problem_params
        self.device = torch.device(device)
        self.head = _HEADS[self.models[0].nn_args["name"]]
        # (one single-model engine per model: problem cache, LazyLinear materialisation and the upper bound are theirs; they
        # allocate nothing until they run)
        self._engines = [FusedRollout(m, problem_params, device) for m in self.models]
        self.small_lane_scenarios = 0   # 16 or 32 scenarios per wavefront (0: small_rollout.lane_width's rule)
        self.last_kernels = {}          # launch class -> kernel name the library recorded in the last run
        self._key = None
        self._shape = _ShapeState(False)   # the current batch shape's buffers and LaunchReplay (read as `ens.rewards`, `ens.plan`, ...)
        self._shapes = {}               # key -> _ShapeState of the other shapes whose launches are replayed
        self.weights = self.grad = self._grad_views = None   # [K][P], [K][P rounded up to 4]: once per engine
        self.param_shapes = None        # shapes of one model's parameters in `parameters()` order (EnsembleAdam's `param_shapes`)
        self._bind_requested = self._bound = False
        self._dims_bound = None         # layer sizes, once the parameters are bound
        self.best_dev = self.best_weights = None   # `fit`: [K] lowest dev loss so far, [K][P] the parameters that gave it

    def __getattr__(self, name):   # (only reached for names the engine itself does not have)
        if name in _ShapeState.FIELDS:
            return getattr(self._shape, name)
        raise AttributeError(name)

    @property
    def n_models(self):
        return len(self.models)

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

    # ---- buffers: weights and gradients once per engine, the rest once per (B, T, K) ---------------------------------------------------
    def _model_buffers(self, dims):
        n_hidden, n_out = len(dims) - 2, dims[-1]
        P = sr.packed_weight_count(dims[0], n_hidden, n_out)
        if self.weights is None:
            self.weights = torch.zeros(self.n_models, P, device=self.device)
            self.param_shapes = [shape for _, n, k, _ in sr.layer_slices(dims[0], n_hidden, n_out) for shape in ((n, k), (n,))]
        assert self.weights.shape[1] == P   # (the models' layer sizes are fixed once they are materialised)

    def _bind(self, lins, dims):
        """weight.data / bias.data of every layer <- views of the model's row of `weights`, which gets the current values once"""
        pack_ensemble_weights(lins, self.weights)
        bind_rows(lins, self.weights, sr.layer_slices(dims[0], len(dims) - 2, dims[-1]))
        self._bound, self._dims_bound = True, dims

    def bind_parameters(self):
        """Opt-in: from now on the models' parameters LIVE in `weights [K][P]` (views of their rows), `run` and `train_step` pack
        nothing, and whatever writes a parameter in place - `load_state_dict`, an optimizer - writes the packed row.  Binds now if
        the input width is known (a materialised first layer), else on the first batch."""
        self._bind_requested = True
        known = materialized_width(self.models)
        if known is not None and not self._bound:
            lins = self._materialized(known)
            dims = self._dims(lins)
            self._model_buffers(dims)
            self._bind(lins, dims)

    def _materialized(self, F):
        for eng in self._engines:
            eng.materialize(F)
        return [eng._linears() for eng in self._engines]

    @staticmethod
    def _dims(lins):
        dims = [[ls[0].in_features] + [m.out_features for m in ls] for ls in lins]
        for i, d in enumerate(dims):
            if d != dims[0]:
                raise ValueError(f"model {i}: layer sizes {d} differ from model 0's {dims[0]}")
        return dims[0]

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
        """Sizes what this batch needs; returns the models' layers (None once the parameters are bound: nothing is packed, and the
        per-model checks were made when they were bound).  `instances`: what the key of a list-of-instances batch carries besides
        the shape (I, the trace length, the tables' layouts); a one-batch run has none."""
        K, dev, ld = self.n_models, self.device, prob.ldb
        F = prob.S * prob.Ws + (0 if self.head == "softplus" else prob.Wn * prob.Ww + prob.E * prob.We)
        if self._bound:
            lins, dims = None, self._dims_bound
        else:
            lins = self._materialized(F)
            dims = self._dims(lins)
        if dims[0] != F or not sr.SmallRolloutPlan.supports(prob, self.head, dims):
            raise ValueError(f"SmallPolicyEnsemble: the whole-horizon kernels do not take this setting / policy (layer sizes {dims}, "
                             f"{F} state rows)")
        if not self._bound:
            self._model_buffers(dims)
            if self._bind_requested:
                self._bind(lins, dims)
                lins = None
        key = (prob.B, T, K, tuple(dims), prob.Ws, prob.Wn, prob.Ww, prob.E, prob.We) + tuple(instances)
        if self._key != key:
            self._switch_shape(key)
        sh = self._shape
        if sh.plan is None:
            sh.plan = plan = sr.SmallRolloutPlan(prob, self.head, dims)
            z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
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
            z = lambda *s_: torch.zeros(*s_, device=dev)  # noqa: E731
            sh.states, sh.hidden, sh.logits = z(K, s["states"]), z(K, s["hidden"]), z(K, s["logits"])
            sh.slab = z(K, s["slab_rows"], s["slab_row_stride"])
            sh.g_reward, sh.g_reward_key = z(ld), None
            if self.grad is None:   # (with the engine's first training run, and kept: it depends on (K, P) only)
                self.grad = z(K, s["grad"])
                self._grad_views = grad_views(self.grad, F, sh.plan.n_hidden, sh.plan.n_out)
            sh.strides.update(states=s["states"], hidden=s["hidden"], logits=s["logits"], slab=s["slab"], grad=s["grad"])
            sh.ens = sr.ensemble_strides(K, **sh.strides)
        return lins

    def param_grads(self):
        """[(parameter, gradient view into the [K][P] buffer of the last training run)] over all models"""
        out = []
        for eng, (gw, gb) in zip(self._engines, self._grad_views):
            for i, m in enumerate(eng._linears()):
                out += [(m.weight, gw[i]), (m.bias, gb[i])]
        return out

    def _note(self, tag):
        name = _lib.lib().nic_last_kernel()
        self.last_kernels[tag] = name.decode() if name else None

    # ---- one batch ---------------------------------------------------------------------------------------------------------------
    def run(self, data, periods, ignore_periods=0, train=True, observation_params=None, demand_soa=None, grad_scale=None,
            accumulate_grads=False, discrete_allocation=False):
        """Rollout of one batch - or, `data` a list of I batches, of instance m // (K // I)'s batch - under every model (and, if
        `train`, d(mean loss)/d(theta) into every model's `param.grad`: views
        into one [K][P] gradient buffer, `accumulate_grads` adds - `small_rollout.assign_grads`).  Arguments as
        `FusedRollout.run`.  Returns (total [K], reported [K]) device tensors; `rewards` [K][T][ldb] holds the per-period costs."""
        if discrete_allocation and train:
            raise ValueError("discrete_allocation is an evaluation-time option of the fused rollout")
        tt = self._step(data, periods, ignore_periods, train, observation_params, demand_soa, grad_scale, discrete_allocation, None)
        if train:
            sr.assign_grads(self.param_grads(), accumulate_grads)
        return tt[:, 0], tt[:, 1]

    def train_step(self, data, periods, ignore_periods=0, optimizer=None, observation_params=None, demand_soa=None, grad_scale=None):
        """One whole training step of all K models (on one batch, or on a list of I instances' batches as in `run`): forward,
        backward, the reduction's two launches and `optimizer`'s two (an
        `EnsembleAdam` over this engine's (K, P)) - no packing, no `param.grad`, no per-model Python.  Needs `bind_parameters()`.
        Returns (total [K], reported [K]) of the step BEFORE the update, as `run` does."""
        self._require_step(optimizer)
        tt = self._step(data, periods, ignore_periods, True, observation_params, demand_soa, grad_scale, False, optimizer)
        return tt[:, 0], tt[:, 1]

    def _fill_state0(self, state0, prob, data):
        """state0 [F][ldb] <- the batch's initial pipelines in the reference's cat(flatten(...)) order"""
        B = prob.B
        a, b = prob.S * prob.Ws, prob.S * prob.Ws + prob.Wn * prob.Ww
        state0[:a].view(prob.S, prob.Ws, -1)[:, :, :B].copy_(data["initial_inventories"].permute(1, 2, 0))
        if self.head != "softplus":
            if prob.Wn:
                state0[a:b].view(prob.Wn, prob.Ww, -1)[:, :, :B].copy_(data["initial_warehouse_inventories"].permute(1, 2, 0))
            if prob.E:
                state0[b:b + prob.E * prob.We].view(prob.E, prob.We, -1)[:, :, :B].copy_(
                    data["initial_echelon_inventories"].permute(1, 2, 0))

    def _step(self, data, periods, ignore_periods, train, observation_params, demand_soa, grad_scale, discrete_allocation, optimizer):
        if isinstance(data, (list, tuple)):
            return self._step_instances(data, periods, ignore_periods, train, observation_params, demand_soa, grad_scale,
                                        discrete_allocation, optimizer)
        lead, dev, K = self._engines[0], self.device, self.n_models
        prob = lead._problem_for(data)
        T, B, ld = periods, prob.B, prob.ldb
        shift = observation_params["demand"]["period_shift"] if observation_params else 0
        if demand_soa is None:
            demand_soa = demand_trace_soa(data["demands"], ld, dev)
        if demand_soa.shape[0] < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        lins = self._setup(prob, T, train)
        if optimizer is not None:
            self._require_optimizer_shape(optimizer)
        sh = self._shape
        replay = sh.replay
        # a captured sequence holds raw pointers: it reads the pinned problem's tables and the staged demand trace, refreshed in place
        prob = replay.pin_problem(prob)
        demand_soa = replay.stage_demand(demand_soa)
        if not self._bound:
            pack_ensemble_weights(lins, self.weights)   # (every run: the optimizers moved the parameters)
        self._fill_state0(sh.state0, prob, data)
        ub = lead._ub() if self.head != "softplus" else 0.0
        width = sr.lane_width(self.small_lane_scenarios, train, B)
        desc = sh.plan.desc(T, shift, self.weights, demand_soa, sh.state0, ub, round_orders=discrete_allocation, prob=prob,
                            lane_scenarios=width)
        hist = (sh.states, sh.hidden, sh.logits) if train else (None, None, None)
        n_el = T * ld
        if train:
            if grad_scale is None:
                grad_scale = 1.0 / (B * T * self.problem_params["n_stores"])
            sh.g_reward_key = sr.set_g_reward(sh.g_reward, B, grad_scale, sh.g_reward_key)

        def launches():
            sr.small_rollout_ensemble_fwd(desc, sh.ens, sh.rewards, sh.final, *hist)
            self._note("fwd")
            if train:
                row = sh.slab.shape[2]
                sr.small_rollout_ensemble_bwd_wgrad(desc, sh.ens, *hist, Table(sh.g_reward, 0, 1), sh.slab, row)
                self._note("bwd")
                sr.small_rollout_ensemble_reduce(sh.ens, sh.slab, sr.slab_rows_written(B, width), row, self.grad.shape[1], self.grad,
                                                 sh.rewards, n_el, ignore_periods * ld, sh.totals, sh.scratch)
            else:   # the same reduction, costs only: an evaluation pass returns the very bits a training pass does
                sr.small_rollout_ensemble_reduce(sh.ens, None, 0, 0, 0, None, sh.rewards, n_el, ignore_periods * ld, sh.totals,
                                                 sh.scratch)
            self._note("reduce")
            if optimizer is not None:
                optimizer.step(self.weights, self.grad)

        # what a captured sequence bakes in besides this shape's buffers.  Engine-wide things are the `variant` (a change drops this
        # shape's captures now, another shape's when it is current again); the optimizer's buffers, which only a training step's
        # sequence holds, are part of the capture's key, so evaluations in between (`fit`) change nothing
        if replay.on():
            replay.set_variant((K, self.small_lane_scenarios, self.weights.data_ptr(), ub))
        opt_key = optimizer and tuple(t.data_ptr() for t in (optimizer.hyper, optimizer.state, optimizer.coef, optimizer.exp_avg,
                                                               optimizer.exp_avg_sq))
        replay.probe_begin(train)
        replay.call((train, opt_key, ignore_periods, shift, bool(discrete_allocation), width), launches)
        replay.probe_end()
        replay.ran()
        return sh.totals.clone()   # (outside the capture: the caller's tensors must not change under a later step)

    def _step_instances(self, datas, periods, ignore_periods, train, observation_params, demand_soa, grad_scale, discrete_allocation,
                        optimizer):
        """`_step` for a list of I batches: model m runs on datas[m // (K // I)].  The instances' inputs are copied into this batch
        shape's stacked buffers (the tables only when the batches present other tensors than last time), whose addresses a captured
        sequence keeps: nothing is pinned or staged."""
        lead, dev, K = self._engines[0], self.device, self.n_models
        I = len(datas)
        if I < 1 or K % I != 0:   # (before anything is built from the batches)
            raise ValueError(f"SmallPolicyEnsemble: {I} problem instances do not divide {K} models")
        probs = [lead._problem_for(data) for data in datas]
        lengths = [int(data["demands"].shape[2]) for data in datas]
        check_instances(probs, K, lengths)
        prob0 = probs[0]
        T, B, ld, T_total = periods, prob0.B, prob0.ldb, lengths[0]
        shift = observation_params["demand"]["period_shift"] if observation_params else 0
        if T_total < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        if demand_soa is not None and tuple(demand_soa.shape) != (I, T_total, 1, ld):
            raise ValueError(f"SmallPolicyEnsemble: demand_soa of a list of instances must be [I][T_total][1][ldb] = {(I, T_total, 1, ld)}, "
                             f"got {tuple(demand_soa.shape)}")
        layouts = tuple((name, getattr(prob0, name).scn_stride) for name in EnvProblem._TABLES if getattr(prob0, name).tensor is not None)
        lins = self._setup(prob0, T, train, instances=("instances", I, T_total, layouts))
        if optimizer is not None:
            self._require_optimizer_shape(optimizer)
        sh = self._shape
        replay = sh.replay
        F = sh.plan.F
        if sh.inst_state0 is None:
            sh.inst_state0 = torch.zeros(I, F, ld, device=dev)
            sh.inst_prob, table_strides = stack_instance_tables(probs)
            sh.inst_sources = probs
            sh.inst = sr.instance_strides(I, state0=F * ld, demand=T_total * ld, **table_strides)
        elif not all(a is b for a, b in zip(sh.inst_sources, probs)):
            for name in EnvProblem._TABLES:   # (other batches than last time: their tables into the stacked ones, in place)
                stacked = getattr(sh.inst_prob, name).tensor
                if stacked is not None:
                    for i, p in enumerate(probs):
                        stacked[i].copy_(getattr(p, name).tensor)
            sh.inst_sources = probs
        if demand_soa is None:
            if sh.inst_demand is None:
                sh.inst_demand = torch.zeros(I, T_total, 1, ld, device=dev)
            demand_soa = sh.inst_demand
            for i, data in enumerate(datas):
                demand_soa[i, :, :, :B].copy_(data["demands"].permute(2, 1, 0))
        if not self._bound:
            pack_ensemble_weights(lins, self.weights)   # (every run: the optimizers moved the parameters)
        for i, data in enumerate(datas):
            self._fill_state0(sh.inst_state0[i], prob0, data)
        ub = lead._ub() if self.head != "softplus" else 0.0
        width = sr.lane_width(self.small_lane_scenarios, train, B)
        desc = sh.plan.desc(T, shift, self.weights, demand_soa, sh.inst_state0, ub, round_orders=discrete_allocation, prob=sh.inst_prob,
                            lane_scenarios=width)
        hist = (sh.states, sh.hidden, sh.logits) if train else (None, None, None)
        n_el = T * ld
        if train:
            if grad_scale is None:
                grad_scale = 1.0 / (B * T * self.problem_params["n_stores"])
            sh.g_reward_key = sr.set_g_reward(sh.g_reward, B, grad_scale, sh.g_reward_key)

        def launches():
            sr.small_rollout_instances_fwd(desc, sh.ens, sh.inst, sh.rewards, sh.final, *hist)
            self._note("fwd")
            if train:
                row = sh.slab.shape[2]
                sr.small_rollout_instances_bwd_wgrad(desc, sh.ens, sh.inst, *hist, Table(sh.g_reward, 0, 1), sh.slab, row)
                self._note("bwd")
                sr.small_rollout_ensemble_reduce(sh.ens, sh.slab, sr.slab_rows_written(B, width), row, self.grad.shape[1], self.grad,
                                                 sh.rewards, n_el, ignore_periods * ld, sh.totals, sh.scratch)
            else:
                sr.small_rollout_ensemble_reduce(sh.ens, None, 0, 0, 0, None, sh.rewards, n_el, ignore_periods * ld, sh.totals,
                                                 sh.scratch)
            self._note("reduce")
            if optimizer is not None:
                optimizer.step(self.weights, self.grad)

        # (as in `_step`; a caller's demand_soa is read in place, so its address is part of the capture's key)
        if replay.on():
            replay.set_variant((K, I, self.small_lane_scenarios, self.weights.data_ptr(), ub))
        opt_key = optimizer and tuple(t.data_ptr() for t in (optimizer.hyper, optimizer.state, optimizer.coef, optimizer.exp_avg,
                                                               optimizer.exp_avg_sq))
        replay.probe_begin(train)
        replay.call((train, opt_key, ignore_periods, shift, bool(discrete_allocation), width, I, demand_soa.data_ptr()), launches)
        replay.probe_end()
        replay.ran()
        return sh.totals.clone()
