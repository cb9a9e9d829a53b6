"""`HorizonPolicyEnsemble`: K `data_driven` policies of ONE architecture (DataDrivenNet, neural_networks.py:430-515) trained or
evaluated on ONE real-data batch with one forward and one backward whole-horizon launch for all of them
(`nic_horizon_rollout_ensemble_*`, csrc/horizon_rollout.hip: grid y = model).

A whole-horizon launch of the reference's real-data batch (72 products x 21 stores x 3 warehouses x 95 weeks) has ceil(72 / 16) = 5
workgroups: a serial chain of 95 periods on 2 % of the device.  Seeds, learning rates or initialisations of one architecture ride in
the idle CUs instead of paying K steps.  Every model runs the instruction stream of the single-model kernels on its own slice of
the buffers, and the four GEMMs around the launch pair (the observation rows' share of the first layer, three weight gradients)
run with the operands, shapes, strides and split counts `FusedRollout`'s whole-horizon route uses - so each model's costs,
final state and gradients are the bits `FusedRollout.run` gives for that model alone (trainer.py:181-216 once per model).  The totals are
one fixed-order reduction for all K models (the cost half of `nic_small_rollout_ensemble_reduce`): they agree with the single-model
`torch.sum` to rounding, not to the bit.

The GEMMs are one launch each for all K models (`nic_linear_fwd_models`, `nic_linear_wgrad_models`, `nic_wgrad_reduce_models`,
csrc/linear_models_plan.h: grid y = model, the single-model plan and kernel on every model's slice, so not a bit of any model's
result changes): one forward, and per layer one `zero_()` of a [K][splits][N][ld] slab, one contraction and one reduction straight
into the [K][P] gradient rows.  `model_gemms = False` - and any shape `ops.linear_models_ok` refuses - takes the per-model loop of
single-model calls instead (4 K GEMM launches + 6 K around them).

`run` alone leaves the optimizer to the caller and packs all K models' weights again every call.  The whole training step is
`train_step`: after `bind_parameters()` every model's `weight` / `bias` are views of its row of `weights [K][P]`, nothing is packed,
and an `EnsembleAdam(K, P)` updates all K rows with two launches - no per-model Python.  `fit` is the epoch loop over `train_step`
with the best weights per model kept on the device.  Packing, binding, the frames of `run` / `train_step`, `fit` and the generic
model checks are `EnsembleStep`'s (ensemble_step.py, shared with `SmallPolicyEnsemble`), model and batch preparation are the
functions every engine calls (policy_layers.py, layout.py: no single-model engine is built here); this module has the policy's
rules, the buffers of a batch shape and the launches.

Layout: weights `[K][P]` in `nn.Linear`'s own order (ensemble_step.py's packed row: per layer the weight, row-major, then the bias;
packed with one `torch.cat` per run unless the parameters are bound), gradients `[K][P]` in the same order (`param.grad` are views of it),
inputs `X [K][F][T][ldb]` (the kernel writes model m's state rows into X[m]; the observation rows are model-independent, filled once
and copied), `z1_obs [K][H1][T][ldb]`, costs `rewards [K][T][ldb]`, histories and pre-activation gradients `[K][rows][T][ldb]`.

The K models need not share the batch: `run`, `train_step` and `fit` take a list (or tuple) of I batch dicts in place of one, I
dividing K, and model m then runs on instance m // (K // I) - its own demand trace, initial state and cost / lead-time tables
(`nic_horizon_rollout_instances_*`: the same launch pair, every model reading its instance's inputs).  That is a sweep of the
underage cost, the lead times or the 72-product slice of a real-data setting, times seeds, in one engine.  The instances share the
topology (the adjacency mask is `problem_params`'), B, the trace length, the pipeline shape (lead times may differ within it), the
flags, the policy's input row count and `period_shift`; `check_instances` names the first mismatch.  The engine owns the
instance-stacked inputs per batch shape (`inst_demand [I][T_total][S][ldb]`, `inst_state0 [I][F_dyn][ldb]`, one stacked tensor per
table); the observation rows are filled once per instance into X[i * R] and copied to its other R - 1 replicas, and the
observation GEMM reads every model's own rows (`X_stride` = one model's slice; its plan is model 0's either way, so no bit of a
model's result depends on which form ran).  The weight-gradient GEMMs, the reductions and the optimizer do not know about
instances.  A plain dict is the one-batch path and calls `nic_horizon_rollout_ensemble_*` as before.

Per-model early stopping (`fit(trainer_params=...)`, `set_active`): a stopped model's weights row and Adam state keep their bits
and its history entries are NaN.  Whether it also leaves the launches is `skip_inactive`, a plain attribute beside `model_gemms`.
False (the default): every launch is the one it always was, whatever the mask - only the optimizer reads it, every model's costs
are computed and the totals are finite.  True, with a mask set: every library launch of a step takes its `_active` entry point
with the mask - the observation GEMM, the forward, the totals reduction, the backward, the three weight-gradient contractions and
their reductions (`nic_horizon_rollout_*_active`, `nic_linear_*_models_active`, `nic_small_rollout_ensemble_reduce_active`), for a
dict batch and for a list of instances - and the totals of the stopped models are NaN, as on `SmallPolicyEnsemble`.  The contract is
that engine's: for a model whose entry is zero no library launch reads or writes its slices - `rewards`, `final`, the state rows
of `X`, the four histories, `dz1..3`, `z1`, its slab, its `grad` row and `totals` row, the reduce scratch, weights, moments and
optimizer state - and a model that runs gets the bits of the unmasked step.  True without a mask: the unmasked launches.
`fit(trainer_params=...)` switches it on for its duration and puts the previous value back.  The per-model loop
(`model_gemms = False`, or a shape the plan refuses) skips the stopped models on the host from `active_models()`: one host read
per step, on that fall-back path only; the launch pair and the totals are masked either way.
The boundary: the torch glue of a step is NOT masked.  It prepares model-independent INPUTS and SCRATCH, not results - the
`W1obs.copy_` of the first layer's observation columns, the copy of the observation rows into the replicas' `X`, `slabs[i].zero_()`
- and runs for all K models as before, so a stopped model's `W1obs` block, observation rows and slab are still written (with what
they would hold anyway).  Glue that follows the mask is not built; tools/horizon_active_step.py times its share of a step.

Not part of this engine: graph replay, per-instance topology / B / horizon, Trainer / YAML / `main_run` wiring, a `torch.library`
operator, multi-GPU sharding, bf16 GEMMs.
"""
import types

import torch

from . import _lib, ops
from . import horizon_rollout as hz
from . import small_rollout as sr
from .ensemble_step import check_instances as _check_problems
from .ensemble_step import (check_model_list, EnsembleStep, grad_views, instance_replicas, layer_slices,
                            refresh_instance_tables, stack_instance_tables, table_layouts)
from .ensemble_step import packed_count, pack_ensemble_weights  # noqa: F401  (re-exports)
from .layout import data_driven_input_rows, demand_trace_soa, edge_mask, fill_initial_state, fill_observation_rows, Table
from .policy_layers import observation_ok
from .rollout import _pad32, FusedRollout  # noqa: F401  (`FusedRollout`: a re-export)


def _layer_sizes(model):
    a = model.nn_args
    return list(a["neurons_per_hidden_layer"]["master"]) + [a["output_sizes"]["master"]]


def check_models(models):
    """The models an ensemble takes: 1 <= K <= 65535 `data_driven` policies `FusedRollout` takes, with the same layer sizes (two
    hidden layers: what the whole-horizon kernels run) and a bias in every layer.  ValueError names the first mismatch.  Host-side
    only; the setting's side of `HorizonPlan.supports` is checked when the first batch arrives."""
    return check_model_list(models, "HorizonPolicyEnsemble", ("data_driven",), "the data_driven policy (ELU inside, ReLU on the output)",
                            _layer_sizes, "layer sizes {} differ from model 0's {}")


def input_rows(prob, data, observation_params):
    """rows of the policy's input for a batch: the state (stores, then warehouses), then the observation rows"""
    return data_driven_input_rows(prob.S * prob.Ws + prob.Wn * prob.Ww, data, observation_params)


def _per_instance(observation_params, n_instances):
    """one observation_params per instance, from one dict for all instances or a list of one per instance"""
    obs = list(observation_params) if isinstance(observation_params, (list, tuple)) else [observation_params] * n_instances
    if len(obs) != n_instances:
        raise ValueError(f"HorizonPolicyEnsemble: {len(obs)} observation_params for {n_instances} problem instances")
    return obs


def check_instances(probs, n_models, datas, observation_params):
    """The problem instances one launch pair takes: I >= 1 batches (their `EnvProblem`s and dicts), I dividing the K models, that
    agree in what the kernels and the GEMMs take once - B, the trace length, the pipeline shape, the flags, every table's presence,
    layout and shape (`ensemble_step.check_instances`), the policy's input row count (past-demand window, time features) and
    `period_shift`.  `observation_params`: one dict for all instances, or one per instance.  ValueError names the first mismatch.
    Host-side only.  Returns the replicas per instance."""
    R = _check_problems(probs, n_models, [int(d["demands"].shape[2]) for d in datas], who="HorizonPolicyEnsemble")
    obs = _per_instance(observation_params, len(probs))
    rows = [input_rows(p, d, o) for p, d, o in zip(probs, datas, obs)]
    for i in range(1, len(probs)):
        if rows[i] != rows[0]:
            raise ValueError(f"instance {i}: the policy's input has {rows[i]} rows (past-demand window, time features), instance 0's {rows[0]}")
        if obs[i]["demand"]["period_shift"] != obs[0]["demand"]["period_shift"]:
            raise ValueError(f"instance {i}: period_shift {obs[i]['demand']['period_shift']} differs from instance 0's "
                             f"{obs[0]['demand']['period_shift']}")
    return R


class HorizonPolicyEnsemble(EnsembleStep):
    def __init__(self, models, problem_params, device):
        super().__init__(check_models(models), problem_params, device)
        self._key = None
        self.plan = self.prob = None
        self._dpad = None               # `fill_observation_rows`' window scratch
        self.model_gemms = True         # one GEMM launch for all K models where the library takes the shape; False: the per-model loop
        self.skip_inactive = False      # True: with a mask set (`set_active`), every library launch of a step skips the stopped models

    def _setup(self, prob, T, train, dims, shift, instances=()):
        """`instances`: what the key of a list-of-instances batch carries besides the shape (I, the trace length, the tables'
        layouts); a one-batch run has none."""
        K, dev, ld = self.n_models, self.device, prob.ldb
        z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        key = (prob.B, T, K, tuple(dims), prob.S, prob.Wn, prob.Ws, prob.Ww, shift) + tuple(instances)
        if self._key != key:
            self._key = None
            for name in ("X", "z1", "W1obs", "hist", "dz", "slabs", "rewards", "final", "state0", "scratch", "totals",
                         "inst_demand", "inst_state0", "inst_prob", "inst", "inst_sources"):
                setattr(self, name, None)   # release the previous shape's buffers before sizing the new ones
            F, FD = dims[0], prob.S * prob.Ws + prob.Wn * prob.Ww
            if not hz.HorizonPlan.supports(prob, "data_driven", dims) or not hz.offsets_ok(prob, T, T + shift, hz.MAX_HIDDEN):
                raise ValueError(f"HorizonPolicyEnsemble: the whole-horizon kernels do not take this setting / policy (layer sizes {dims}, "
                                 f"{FD} state rows, {prob.B} scenarios x {T} periods)")
            self.plan = hz.HorizonPlan(prob, dims)
            self._model_buffers(dims)
            self.F, self.F_dyn, self.dims = F, FD, list(dims)
            self.state0 = z(FD, ld)
            self.rewards, self.final = z(K, T, ld), z(K, FD, ld)
            self.X = z(K, F, T, ld)       # rows [0, FD): state before period t (written by the kernel); then the observation rows
            self.z1 = z(K, dims[1], T, ld)
            self.W1obs = z(K, dims[1], _pad32(F - FD))   # (rows padded to 32 floats, as FusedRollout's: the GEMM's A-tile loads are float4)
            self.edge_mask = edge_mask(self.problem_params, dev)
            self.totals = z(K, 2)
            n_scratch = sr.small_rollout_reduce_scratch(0, 0, T * ld)
            self.scratch = torch.empty(K, n_scratch, device=dev)
            self._reduce = sr.ensemble_strides(K, rewards=T * ld, scratch=n_scratch)
            self._strides = None
            self._checked = False
            # once per shape: do the model-batched GEMMs take it (the first layer's observation share, three one-period weight
            # gradients over T * ld columns)?  If not, `run` takes the per-model loop.
            n_cols = T * ld
            self._models_ok = (ops.linear_models_ok(dims[1], F - FD, n_cols, n_cols, K)
                               and all(ops.linear_models_ok(dims[i + 1], dims[i], n_cols, n_cols, K, wgrad=True) for i in range(3)))
            self._key = key
        if train and self.hist is None:
            # the training buffers come with the first training run of a shape and stay: evaluation runs in between use the rest
            n_cols = T * ld
            rows = [dims[1], dims[2], dims[3], self.plan.n_ord + prob.Wn]   # h1, h2, logits, orders (+ shipped)
            self.hist = [z(K, r, T, ld) for r in rows]
            self.dz = [z(K, dims[i + 1], T, ld) for i in range(3)]   # (padding columns stay zero: the kernel writes live ones only)
            self.g_reward, self._g_reward_key = z(ld), None
            # (a slab per model: one launch contracts a layer for all K; the per-model loop uses model 0's, one contraction after the other)
            self.splits = [ops.wgrad_num_splits(dims[i + 1], dims[i], n_cols) for i in range(3)]
            self.slabs = [z(K, self.splits[i], dims[i + 1], (dims[i] + 1 + 3) // 4 * 4) for i in range(3)]
            if self.grad is None:
                self.grad = z(K, self.weights.shape[1])
                self._grad_views = grad_views(self.grad, dims)
            self._strides = None

    def _ensemble(self, desc, train):
        """NicHorizonEnsemble of the current buffers, checked once per shape against csrc/horizon_ensemble_plan.h's slices"""
        if self._strides is None or self._strides[0] != bool(train):
            P = self.weights.shape[1]
            st = dict(W1=P, W2=P, W3=P, b2=P, b3=P, z1_obs=self.z1[0].numel(), rewards=self.rewards[0].numel(),
                      state_final=self.final[0].numel())
            if train:
                st.update(state_hist=self.X[0].numel(), h1_hist=self.hist[0][0].numel(), h2_hist=self.hist[1][0].numel(),
                          logits_hist=self.hist[2][0].numel(), orders_hist=self.hist[3][0].numel(), dz1=self.dz[0][0].numel(),
                          dz2=self.dz[1][0].numel(), dz3=self.dz[2][0].numel())
            sl = hz.ensemble_slices(desc)
            assert all(v >= sl[k] for k, v in st.items()), (st, sl)
            self._strides = (bool(train), hz.ensemble_strides(self.n_models, **st))
        return self._strides[1]

    # ---- one batch ---------------------------------------------------------------------------------------------------------------
    def run(self, data, periods, ignore_periods=0, train=True, observation_params=None, grad_scale=None, accumulate_grads=False,
            discrete_allocation=False):
        """Rollout of one batch - or, `data` a list of I batches, of instance m // (K // I)'s batch - under every model (and, if
        `train`, d(mean loss)/d(theta) into every model's `param.grad`: views into one [K][P] gradient buffer, `accumulate_grads`
        adds - `small_rollout.assign_grads`).  Arguments as `FusedRollout.run`.
        Returns (total [K], reported [K]) device tensors; `rewards` [K][T][ldb] holds the per-period costs.  A setting the
        whole-horizon kernels do not take is a ValueError: there is no fall-back to K single steps."""
        return self._run((data, periods, ignore_periods, observation_params, grad_scale), train, accumulate_grads, discrete_allocation)

    def train_step(self, data, periods, ignore_periods=0, optimizer=None, observation_params=None, grad_scale=None):
        """One whole training step of all K models (on one batch, or on a list of I instances' batches as in `run`): forward, the
        cost reduction, backward, the batched weight gradients and `optimizer.step(self.weights, self.grad)` (an `EnsembleAdam`
        over this engine's (K, P)) - no packing, no `param.grad`, no
        per-model Python.  Needs `bind_parameters()`.  Returns (total [K], reported [K]) of the step BEFORE the update, as `run`
        does."""
        return self._train_step((data, periods, ignore_periods, observation_params, grad_scale), optimizer)

    def _stage_instances(self, datas, probs, T_total):
        """A list of I batches: the instances' traces, initial states and tables into this batch shape's stacked buffers (the tables
        only when the batches present other tensors than last time).  Returns (the problem, demand trace and initial state the
        descriptor points at - instance 0's, instance i's i x a stride behind) and the NicHorizonInstances."""
        prob0, dev, I = probs[0], self.device, len(probs)
        B, ld, FD = prob0.B, prob0.ldb, self.F_dyn
        if self.inst_state0 is None:
            self.inst_state0 = torch.zeros(I, FD, ld, device=dev)
            self.inst_demand = torch.zeros(I, T_total, prob0.S, ld, device=dev)
            self.inst_prob, table_strides = stack_instance_tables(probs)
            self.inst_sources = probs
            self.inst = hz.instance_strides(I, state0=FD * ld, demand=T_total * prob0.S * ld, **table_strides)
        else:   # (other batches than last time: their tables into the stacked ones, in place)
            self.inst_sources = refresh_instance_tables(self.inst_prob, self.inst_sources, probs)
        for i, data in enumerate(datas):
            self.inst_demand[i, :, :, :B].copy_(data["demands"].permute(2, 1, 0))
            fill_initial_state(self.inst_state0[i], prob0, data)
        return (self.inst_prob, self.inst_demand, self.inst_state0), self.inst

    def _step(self, data, periods, ignore_periods, observation_params, grad_scale, train, discrete_allocation, optimizer):
        """`data` a dict: all K models on one batch (`nic_horizon_rollout_ensemble_*`); a list or tuple of I dicts: model m on its
        instance's (`nic_horizon_rollout_instances_*`, also for I = 1).  The kind of input decides the staging and the launch pair's
        entry points; the rest is one path."""
        dev, K = self.device, self.n_models
        listed = isinstance(data, (list, tuple))
        if listed:
            datas = list(data)
            I = len(datas)
            instance_replicas(I, K, "HorizonPolicyEnsemble")   # (this and the next: before anything is built from the batches)
            obs = _per_instance(observation_params, I)
            for d, o in zip(datas, obs):
                if not observation_ok(self.models[0], o, d):
                    raise ValueError("data_driven needs a past-demand window and the days_from_christmas time feature")
            probs = [self._problem_for(d) for d in datas]
            R = check_instances(probs, K, datas, obs)
            observation_params = obs[0]
        else:   # (one batch: nothing to compare, no per-instance Python)
            if not observation_ok(self.models[0], observation_params, data):
                raise ValueError("data_driven needs a past-demand window and the days_from_christmas time feature")
            datas, probs, obs, I, R = (data,), (self._problem_for(data),), (observation_params,), 1, K
        prob = self.prob = probs[0]
        T, B, ld = periods, prob.B, prob.ldb
        shift = observation_params["demand"]["period_shift"]
        FD = prob.S * prob.Ws + prob.Wn * prob.Ww
        F = input_rows(prob, datas[0], observation_params)
        lins, dims = self._layers(F)
        if self._bound and dims[0] != F:
            raise ValueError(f"HorizonPolicyEnsemble: this batch gives the policy {F} input rows, the bound parameters have {dims[0]}")
        if prob.E != 0 or len(dims) != 4:
            raise ValueError(f"HorizonPolicyEnsemble: the whole-horizon kernels do not take this setting / policy (layer sizes {dims}, "
                             f"{prob.E} extra echelons)")
        T_total = int(datas[0]["demands"].shape[2])
        if T_total < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        if listed:
            self._setup(prob, T, train, dims, shift, instances=("instances", I, T_total, table_layouts(prob)))
        else:
            self._setup(prob, T, train, dims, shift)
        self._ready_weights(lins, dims, optimizer)
        Fo, n_cols = F - FD, T * ld
        batched = self.model_gemms and self._models_ok
        # the stopped models leave the launches only on request (`skip_inactive`) and only once a mask is set; else every launch is
        # the unmasked one.  The per-model loops then run the models that are active (one host read, on that path only)
        mask = self._mask() if self.skip_inactive else None
        masked = {} if mask is None else {"active": mask}
        running = range(K) if mask is None or batched else [m for m, on in enumerate(self.active_models().tolist()) if on]
        P, sl = self.weights.shape[1], layer_slices(dims)
        if listed:
            (prob_d, demand_soa, state0), inst = self._stage_instances(datas, probs, T_total)
            traces = demand_soa
        else:
            prob_d, demand_soa, state0, inst = prob, demand_trace_soa(data["demands"], ld, dev), self.state0, None
            traces = demand_soa.unsqueeze(0)
            fill_initial_state(state0, prob, data)
        # the observation rows do not depend on the model: filled once per instance (the routine `FusedRollout` uses) into its first
        # replica's block, then one copy to every instance's other R - 1
        X = self.X
        for i, (d, p, o) in enumerate(zip(datas, probs, obs)):
            P_ = o["demand"]["past_periods"]
            shape = (P_ + traces[i].shape[0], p.S, p.ldb)
            if self._dpad is None or self._dpad.shape != shape:
                self._dpad = torch.zeros(shape, device=dev)
            end = fill_observation_rows(X[i * R].transpose(0, 1), FD, p.S, P_, T, p.B, shift, d, traces[i], self._dpad)
            assert end == F
        if R > 1:
            Xi = X.view(I, R, F, T, ld)
            Xi[:, 1:, FD:].copy_(Xi[:, :1, FD:].expand(I, R - 1, Fo, T, ld))
        # with the single-model route's operands: the observation rows' share of the first layer for every period (+ bias)
        row0 = self.weights[0]
        if batched:
            # one strided copy and one launch: the weights and biases are read in the packed rows; the observation rows are shared
            # (one batch: X stride 0) or every model's own block's (a list of instances: X stride = one model's slice of X)
            o, n, k, bo = sl[0]
            self.W1obs[:, :, :Fo].copy_(self.weights[:, o:o + n * k].view(K, n, k)[:, :, FD:])
            x_obs = X[:, FD:].flatten(2) if listed else X[0, FD:].view(Fo, n_cols)
            ops.linear_fwd_models(self.W1obs[:, :, :Fo], row0[bo:bo + n], x_obs, self.z1.view(K, dims[1], n_cols),
                                  n_cols, _lib.NIC_ACT_NONE, bias_stride=P, **masked)
        else:
            linears = lins or self._linears()
            for m in running:
                ls = linears[m]
                self.W1obs[m, :, :Fo].copy_(ls[0].weight.detach()[:, FD:])
                ops.linear_fwd(self.W1obs[m, :, :Fo], ls[0].bias.detach(), X[m, FD:].view(Fo, n_cols), self.z1[m].view(dims[1], n_cols),
                               n_cols, _lib.NIC_ACT_NONE)
        self._note("z1")
        # the descriptor points at model 0's row of the packed weights
        views = [types.SimpleNamespace(weight=row0[o:o + n * k].view(n, k), bias=row0[bo:bo + n]) for o, n, k, bo in sl]
        desc = self.plan.desc(prob_d, T, shift, views, self.edge_mask, demand_soa, n_cols, round_orders=discrete_allocation)
        if not self._checked:   # once per shape: the library's own limits
            if not hz.horizon_ok(desc):
                msg = _lib.lib().nic_last_error()
                raise ValueError("HorizonPolicyEnsemble: the whole-horizon kernels do not take this shape: " + (msg.decode() if msg else "?"))
            self._checked = True
        ens = self._ensemble(desc, train)
        hist = ([X] + self.hist) if train else [None] * 5
        if inst is None:
            fwd, bwd, where = hz.horizon_ensemble_fwd, hz.horizon_ensemble_bwd, (desc, ens)
        else:
            fwd, bwd, where = hz.horizon_instances_fwd, hz.horizon_instances_bwd, (desc, ens, inst)
        fwd(*where, self.z1, state0, self.rewards, self.final, *hist, **masked)
        self._note("fwd")
        # every model's total / reported cost: one fixed-order reduction (two launches) for all K
        sr.small_rollout_ensemble_reduce(self._reduce, None, 0, 0, 0, None, self.rewards, n_cols, ignore_periods * ld, self.totals,
                                         self.scratch, **masked)
        tt = self.totals.clone()   # (the caller's tensors must not change under a later run)
        if mask is not None:       # (the reduction left the stopped models' rows alone: what stands there is an earlier run's)
            tt = self._mask_totals(tt)
        if not train:
            return tt
        if grad_scale is None:
            grad_scale = 1.0 / (B * T * self.problem_params["n_stores"])
        self._g_reward_key = sr.set_g_reward(self.g_reward, B, grad_scale, self._g_reward_key)
        bwd(*where, *hist, Table(self.g_reward, 0, 1), *self.dz, **masked)
        self._note("bwd")
        # three weight gradients per model: FusedRollout._wgrad_over_columns' launches on model m's slices
        if batched:
            for i, x in enumerate((X, self.hist[0], self.hist[1])):   # per layer, all K models: zero, contract, reduce into grad[:, ...]
                o, n, k, bo = sl[i]
                self.slabs[i].zero_()
                ops.linear_wgrad_models(self.dz[i].flatten(2), x.flatten(2), self.slabs[i], n_cols, **masked)
                self._note("wgrad%d" % i)
                ops.wgrad_reduce_models(self.slabs[i], self.grad[0, o:o + n * k].view(n, k), self.grad[0, bo:bo + n], k, 1.0,
                                        dW_stride=P, db_stride=P, **masked)
                self._note("reduce%d" % i)
        else:
            for m in running:
                gw, gb = self._grad_views[m]
                inputs = [X[m], self.hist[0][m], self.hist[1][m]]
                for i, x in enumerate(inputs):
                    slab = self.slabs[i][0]
                    slab.zero_()
                    ops.linear_wgrad(self.dz[i][m].flatten(1), x.flatten(1), slab, n_cols)
                    if m == running[0]:   # (the K models of a layer run the same kernel: noted once)
                        self._note("wgrad%d" % i)
                    ops.wgrad_reduce(slab, gw[i], gb[i], dims[i], 1.0)
                    if m == running[0]:
                        self._note("reduce%d" % i)
        if optimizer is not None:   # (reads the active-model mask whatever `skip_inactive` says: a stopped model's row is frozen)
            mask = self._mask()
            optimizer.step(self.weights, self.grad, **({} if mask is None else {"active": mask}))
        return tt

    # ---- inspection helpers used by the parity tests --------------------------------------------------------------------------------
    def per_period_rewards(self):
        """[K][T][B]"""
        return self.rewards[:, :, :self.prob.B]

    def final_state(self, m):
        """model m's state after the last period, as `FusedRollout.final_state`"""
        from .layout import ref_view
        prob, a = self.prob, self.prob.S * self.prob.Ws
        out = {"store_inventories": ref_view(self.final[m, :a].view(prob.S, prob.Ws, -1), prob.B)}
        if prob.Wn:
            out["warehouse_inventories"] = ref_view(self.final[m, a:].view(prob.Wn, prob.Ww, -1), prob.B)
        return out
