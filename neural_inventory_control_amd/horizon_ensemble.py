"""`HorizonPolicyEnsemble`: K `data_driven` policies of ONE architecture (DataDrivenNet, neural_networks.py:430-515) trained or
evaluated on ONE real-data batch with one forward and one backward whole-horizon launch for all of them
(`nic_horizon_rollout_ensemble_*`, csrc/horizon_rollout.hip: grid y = model).

A whole-horizon launch of the reference's real-data batch (72 products x 21 stores x 3 warehouses x 95 weeks) has ceil(72 / 16) = 5
workgroups: a serial chain of 95 periods on 2 % of the device.  Seeds, learning rates or initialisations of one architecture ride in
the idle CUs instead of paying K steps.  Every model runs the instruction stream of the single-model kernels on its own slice of
the buffers, and the four GEMMs around the launch pair (the observation rows' share of the first layer, three weight gradients)
run with the operands, shapes, strides and split counts `FusedRollout`'s whole-horizon route uses - so each model's costs,
final state and gradients are the bits `FusedRollout(model).run` gives for it (trainer.py:181-216 once per model).  The totals are
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
model checks are `EnsembleStep`'s (ensemble_step.py, shared with `SmallPolicyEnsemble`); this module has the policy's rules, the
buffers of a batch shape and the launches.

Layout: weights `[K][P]` in `nn.Linear`'s own order (ensemble_step.py's packed row: per layer the weight, row-major, then the bias;
packed with one `torch.cat` per run unless the parameters are bound), gradients `[K][P]` in the same order (`param.grad` are views of it),
inputs `X [K][F][T][ldb]` (the kernel writes model m's state rows into X[m]; the observation rows are model-independent, filled once
and copied), `z1_obs [K][H1][T][ldb]`, costs `rewards [K][T][ldb]`, histories and pre-activation gradients `[K][rows][T][ldb]`.

Not part of this engine: graph replay, problem instances per model, Trainer / YAML / `main_run` wiring, a `torch.library` operator,
multi-GPU sharding, bf16 GEMMs.
"""
import types

import torch

from . import _lib, ops
from . import horizon_rollout as hz
from . import small_rollout as sr
from .ensemble_step import (check_model_list, EnsembleStep, grad_views, layer_slices,  # noqa: F401  (the last two: re-exports)
                            packed_count, pack_ensemble_weights)
from .layout import demand_trace_soa, Table
from .rollout import _pad32, FusedRollout


def _layer_sizes(model):
    a = model.nn_args
    return list(a["neurons_per_hidden_layer"]["master"]) + [a["output_sizes"]["master"]]


def check_models(models):
    """The models an ensemble takes: 1 <= K <= 65535 `data_driven` policies `FusedRollout` takes, with the same layer sizes (two
    hidden layers: what the whole-horizon kernels run) and a bias in every layer.  ValueError names the first mismatch.  Host-side
    only; the setting's side of `HorizonPlan.supports` is checked when the first batch arrives."""
    return check_model_list(models, "HorizonPolicyEnsemble", ("data_driven",), "the data_driven policy (ELU inside, ReLU on the output)",
                            _layer_sizes, "layer sizes {} differ from model 0's {}")


class HorizonPolicyEnsemble(EnsembleStep):
    def __init__(self, models, problem_params, device):
        super().__init__(check_models(models), problem_params, device)
        self._key = None
        self.plan = self.prob = None
        self.model_gemms = True         # one GEMM launch for all K models where the library takes the shape; False: the per-model loop

    def _setup(self, prob, T, train, dims, shift):
        K, dev, ld = self.n_models, self.device, prob.ldb
        z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        key = (prob.B, T, K, tuple(dims), prob.S, prob.Wn, prob.Ws, prob.Ww, shift)
        if self._key != key:
            self._key = None
            for name in ("X", "z1", "W1obs", "hist", "dz", "slabs", "rewards", "final", "state0", "scratch", "totals"):
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
            if prob.Wn:
                conn = self.problem_params["warehouse_store_adjacency"]
                self.edge_mask = torch.tensor(conn, dtype=torch.float32, device=dev).t().contiguous()   # [S][Wn]
            else:
                self.edge_mask = None
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
        """Rollout of one batch under every model (and, if `train`, d(mean loss)/d(theta) into every model's `param.grad`: views
        into one [K][P] gradient buffer, `accumulate_grads` adds - `small_rollout.assign_grads`).  Arguments as `FusedRollout.run`.
        Returns (total [K], reported [K]) device tensors; `rewards` [K][T][ldb] holds the per-period costs.  A setting the
        whole-horizon kernels do not take is a ValueError: there is no fall-back to K single steps."""
        return self._run((data, periods, ignore_periods, observation_params, grad_scale), train, accumulate_grads, discrete_allocation)

    def train_step(self, data, periods, ignore_periods=0, optimizer=None, observation_params=None, grad_scale=None):
        """One whole training step of all K models: forward, the cost reduction, backward, the batched weight gradients and
        `optimizer.step(self.weights, self.grad)` (an `EnsembleAdam` over this engine's (K, P)) - no packing, no `param.grad`, no
        per-model Python.  Needs `bind_parameters()`.  Returns (total [K], reported [K]) of the step BEFORE the update, as `run`
        does."""
        return self._train_step((data, periods, ignore_periods, observation_params, grad_scale), optimizer)

    def _step(self, data, periods, ignore_periods, observation_params, grad_scale, train, discrete_allocation, optimizer):
        lead, dev, K = self._engines[0], self.device, self.n_models
        if not FusedRollout.observation_ok(self.models[0], observation_params, data):
            raise ValueError("data_driven needs a past-demand window and the days_from_christmas time feature")
        prob = self.prob = lead._problem_for(data)
        T, B, ld = periods, prob.B, prob.ldb
        shift = observation_params["demand"]["period_shift"]
        P_ = observation_params["demand"]["past_periods"]
        FD = prob.S * prob.Ws + prob.Wn * prob.Ww
        F = FD + prob.S * P_ + 2 * prob.S + data["days_from_christmas"].shape[1] + prob.S * data["lead_times"].shape[2]
        lins, dims = self._layers(F)
        if self._bound and dims[0] != F:
            raise ValueError(f"HorizonPolicyEnsemble: this batch gives the policy {F} input rows, the bound parameters have {dims[0]}")
        if prob.E != 0 or len(dims) != 4:
            raise ValueError(f"HorizonPolicyEnsemble: the whole-horizon kernels do not take this setting / policy (layer sizes {dims}, "
                             f"{prob.E} extra echelons)")
        demand_soa = demand_trace_soa(data["demands"], ld, dev)
        if demand_soa.shape[0] < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        self._setup(prob, T, train, dims, shift)
        self._ready_weights(lins, dims, optimizer)
        Fo, n_cols = F - FD, T * ld
        batched = self.model_gemms and self._models_ok
        P, sl = self.weights.shape[1], layer_slices(dims)
        a = prob.S * prob.Ws
        self.state0[:a].view(prob.S, prob.Ws, ld)[:, :, :B].copy_(data["initial_inventories"].permute(1, 2, 0))
        if prob.Wn:
            self.state0[a:].view(prob.Wn, prob.Ww, ld)[:, :, :B].copy_(data["initial_warehouse_inventories"].permute(1, 2, 0))
        # the observation rows are the same for every model: filled once (FusedRollout's own routine), copied to the other K - 1
        X = self.X
        lead.F, lead.F_dyn = F, FD   # (what the routine reads of its engine besides the window scratch it keeps: the row counts)
        lead._fill_observation_rows(X[0].transpose(0, 1), data, prob, T, shift, observation_params, demand_soa)
        if K > 1:
            X[1:, FD:].copy_(X[0, FD:].unsqueeze(0).expand(K - 1, Fo, T, ld))
        # with the single-model route's operands: the observation rows' share of the first layer for every period (+ bias)
        row0 = self.weights[0]
        if batched:
            # one strided copy and one launch: the weights and biases are read in the packed rows, the observation rows are shared
            o, n, k, bo = sl[0]
            self.W1obs[:, :, :Fo].copy_(self.weights[:, o:o + n * k].view(K, n, k)[:, :, FD:])
            ops.linear_fwd_models(self.W1obs[:, :, :Fo], row0[bo:bo + n], X[0, FD:].view(Fo, n_cols), self.z1.view(K, dims[1], n_cols),
                                  n_cols, _lib.NIC_ACT_NONE, bias_stride=P)
        else:
            for m, ls in enumerate(lins or [eng._linears() for eng in self._engines]):
                self.W1obs[m, :, :Fo].copy_(ls[0].weight.detach()[:, FD:])
                ops.linear_fwd(self.W1obs[m, :, :Fo], ls[0].bias.detach(), X[m, FD:].view(Fo, n_cols), self.z1[m].view(dims[1], n_cols),
                               n_cols, _lib.NIC_ACT_NONE)
        self._note("z1")
        # the descriptor points at model 0's row of the packed weights
        views = [types.SimpleNamespace(weight=row0[o:o + n * k].view(n, k), bias=row0[bo:bo + n]) for o, n, k, bo in sl]
        desc = self.plan.desc(prob, T, shift, views, self.edge_mask, demand_soa, n_cols, round_orders=discrete_allocation)
        if not self._checked:   # once per shape: the library's own limits
            if not hz.horizon_ok(desc):
                msg = _lib.lib().nic_last_error()
                raise ValueError("HorizonPolicyEnsemble: the whole-horizon kernels do not take this shape: " + (msg.decode() if msg else "?"))
            self._checked = True
        ens = self._ensemble(desc, train)
        hist = ([X] + self.hist) if train else [None] * 5
        hz.horizon_ensemble_fwd(desc, ens, self.z1, self.state0, self.rewards, self.final, *hist)
        self._note("fwd")
        # every model's total / reported cost: one fixed-order reduction (two launches) for all K
        sr.small_rollout_ensemble_reduce(self._reduce, None, 0, 0, 0, None, self.rewards, n_cols, ignore_periods * ld, self.totals,
                                         self.scratch)
        tt = self.totals.clone()   # (the caller's tensors must not change under a later run)
        if not train:
            return tt
        if grad_scale is None:
            grad_scale = 1.0 / (B * T * self.problem_params["n_stores"])
        self._g_reward_key = sr.set_g_reward(self.g_reward, B, grad_scale, self._g_reward_key)
        hz.horizon_ensemble_bwd(desc, ens, *hist, Table(self.g_reward, 0, 1), *self.dz)
        self._note("bwd")
        # three weight gradients per model: FusedRollout._wgrad_over_columns' launches on model m's slices
        if batched:
            for i, x in enumerate((X, self.hist[0], self.hist[1])):   # per layer, all K models: zero, contract, reduce into grad[:, ...]
                o, n, k, bo = sl[i]
                self.slabs[i].zero_()
                ops.linear_wgrad_models(self.dz[i].flatten(2), x.flatten(2), self.slabs[i], n_cols)
                self._note("wgrad%d" % i)
                ops.wgrad_reduce_models(self.slabs[i], self.grad[0, o:o + n * k].view(n, k), self.grad[0, bo:bo + n], k, 1.0,
                                        dW_stride=P, db_stride=P)
                self._note("reduce%d" % i)
        else:
            for m, (gw, gb) in enumerate(self._grad_views):
                inputs = [X[m], self.hist[0][m], self.hist[1][m]]
                for i, x in enumerate(inputs):
                    slab = self.slabs[i][0]
                    slab.zero_()
                    ops.linear_wgrad(self.dz[i][m].flatten(1), x.flatten(1), slab, n_cols)
                    if m == 0:   # (the K models of a layer run the same kernel: noted once)
                        self._note("wgrad%d" % i)
                    ops.wgrad_reduce(slab, gw[i], gb[i], dims[i], 1.0)
                    if m == 0:
                        self._note("reduce%d" % i)
        if optimizer is not None:
            optimizer.step(self.weights, self.grad)
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
