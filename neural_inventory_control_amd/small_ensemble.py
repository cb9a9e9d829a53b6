"""`SmallPolicyEnsemble`: K small policies of ONE architecture (`vanilla_one_store` / `vanilla_serial`, 32-wide MLPs) trained or
evaluated on ONE batch with one forward launch, one backward launch and one reduction for all of them
(`nic_small_rollout_ensemble_*`, csrc/small_rollout16.hip / small_rollout.hip / small_reduce.hip: grid y = model).

A wavefront of the whole-horizon kernels is one serial chain of T periods, and at the batch sizes these policies are trained
with (1,024 - 8,192 scenarios) most SIMDs have no wavefront: seeds, learning rates or initialisations of one architecture ride
in them instead of paying K steps.  Every model runs the instruction stream of the single-model kernels on its own slice of the
buffers, so its costs and gradients are the bits `FusedRollout(model).run` gives for it (trainer.py:181-216 once per model).

The launches are eager.  Graph replay, `Trainer` integration, a `torch.library` operator and multi-GPU sharding are not part of
this engine; the engine owns no optimizer (K optimizers, or one with K parameter groups, step the models independently).
"""
import torch

from . import _lib
from . import small_rollout as sr
from .layout import demand_trace_soa, Table
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


class SmallPolicyEnsemble:
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
        self.plan = None
        self.states = None
        self._key = None

    @property
    def n_models(self):
        return len(self.models)

    # ---- buffers: once per (B, T, K) ---------------------------------------------------------------------------------------------
    def _setup(self, prob, T, train):
        K, dev, ld = self.n_models, self.device, prob.ldb
        F = prob.S * prob.Ws + (0 if self.head == "softplus" else prob.Wn * prob.Ww + prob.E * prob.We)
        for eng in self._engines:
            eng.materialize(F)
        lins = [eng._linears() for eng in self._engines]
        dims = [[ls[0].in_features] + [m.out_features for m in ls] for ls in lins]
        for i, d in enumerate(dims):
            if d != dims[0]:
                raise ValueError(f"model {i}: layer sizes {d} differ from model 0's {dims[0]}")
        if dims[0][0] != F or not sr.SmallRolloutPlan.supports(prob, self.head, dims[0]):
            raise ValueError(f"SmallPolicyEnsemble: the whole-horizon kernels do not take this setting / policy (layer sizes {dims[0]}, "
                             f"{F} state rows)")
        key = (prob.B, T, K, tuple(dims[0]), prob.Ws, prob.Wn, prob.Ww, prob.E, prob.We)
        if self._key != key:
            for name in ("states", "hidden", "logits", "slab", "grad", "scratch"):
                setattr(self, name, None)   # release the previous shapes' buffers before sizing the new ones
            self.plan = plan = sr.SmallRolloutPlan(prob, self.head, dims[0])
            z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
            self.weights = z(K, sr.packed_weight_count(F, plan.n_hidden, plan.n_out))
            self.state0 = z(F, ld)
            self.rewards, self.final = z(K, T, ld), z(K, F, ld)
            self.totals = z(K, 2)
            # slice sizes: csrc/small_ensemble_plan.h through the library.  Histories and slab are sized for 16 scenarios per
            # wavefront (as FusedRollout sizes them: the 32-wide form uses the first F / n_out rows and half the slab rows)
            probe = plan.desc(T, 0, self.weights, self.state0, self.state0, 0.0, prob=prob, lane_scenarios=16)
            self.slices = s = sr.ensemble_slices(probe)
            assert s["weights"] == self.weights.shape[1] and s["rewards"] == T * ld and s["final_state"] == F * ld
            self.scratch = torch.empty(K, s["scratch"], device=dev)   # (a training step's need; the cost sums alone use less)
            self.strides = dict(weights=s["weights"], rewards=s["rewards"], final_state=s["final_state"], scratch=s["scratch"])
            self.ens = sr.ensemble_strides(K, **self.strides)
            self._key = key
        if train and self.states is None:
            # the training buffers come with the first training run of a shape and stay: evaluation runs in between use the rest
            s, plan = self.slices, self.plan
            z = lambda *s_: torch.zeros(*s_, device=dev)  # noqa: E731
            self.states, self.hidden, self.logits = z(K, s["states"]), z(K, s["hidden"]), z(K, s["logits"])
            self.slab, self.grad = z(K, s["slab_rows"], s["slab_row_stride"]), z(K, s["grad"])
            self.g_reward, self._g_reward_key = z(ld), None
            self.strides.update(states=s["states"], hidden=s["hidden"], logits=s["logits"], slab=s["slab"], grad=s["grad"])
            self._grad_views = grad_views(self.grad, F, plan.n_hidden, plan.n_out)
            self.ens = sr.ensemble_strides(K, **self.strides)
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
        """Rollout of one batch under every model (and, if `train`, d(mean loss)/d(theta) into every model's `param.grad`: views
        into one [K][P] gradient buffer, `accumulate_grads` adds - `small_rollout.assign_grads`).  Arguments as
        `FusedRollout.run`.  Returns (total [K], reported [K]) device tensors; `rewards` [K][T][ldb] holds the per-period costs."""
        if discrete_allocation and train:
            raise ValueError("discrete_allocation is an evaluation-time option of the fused rollout")
        lead, dev, K = self._engines[0], self.device, self.n_models
        prob = lead._problem_for(data)
        T, B, ld = periods, prob.B, prob.ldb
        shift = observation_params["demand"]["period_shift"] if observation_params else 0
        if demand_soa is None:
            demand_soa = demand_trace_soa(data["demands"], ld, dev)
        if demand_soa.shape[0] < T + shift:
            raise ValueError("Current period is greater than the number of periods in the data")
        lins = self._setup(prob, T, train)
        pack_ensemble_weights(lins, self.weights)   # (every run: the optimizers moved the parameters)
        a, b = prob.S * prob.Ws, prob.S * prob.Ws + prob.Wn * prob.Ww
        self.state0[:a].view(prob.S, prob.Ws, -1)[:, :, :B].copy_(data["initial_inventories"].permute(1, 2, 0))
        if self.head != "softplus":
            if prob.Wn:
                self.state0[a:b].view(prob.Wn, prob.Ww, -1)[:, :, :B].copy_(data["initial_warehouse_inventories"].permute(1, 2, 0))
            if prob.E:
                self.state0[b:b + prob.E * prob.We].view(prob.E, prob.We, -1)[:, :, :B].copy_(
                    data["initial_echelon_inventories"].permute(1, 2, 0))
        ub = lead._ub() if self.head != "softplus" else 0.0
        width = sr.lane_width(self.small_lane_scenarios, train, B)
        desc = self.plan.desc(T, shift, self.weights, demand_soa, self.state0, ub, round_orders=discrete_allocation, prob=prob,
                              lane_scenarios=width)
        hist = (self.states, self.hidden, self.logits) if train else (None, None, None)
        sr.small_rollout_ensemble_fwd(desc, self.ens, self.rewards, self.final, *hist)
        self._note("fwd")
        n_el = T * ld
        if train:
            if grad_scale is None:
                grad_scale = 1.0 / (B * T * self.problem_params["n_stores"])
            self._g_reward_key = sr.set_g_reward(self.g_reward, B, grad_scale, self._g_reward_key)
            row = self.slab.shape[2]
            sr.small_rollout_ensemble_bwd_wgrad(desc, self.ens, *hist, Table(self.g_reward, 0, 1), self.slab, row)
            self._note("bwd")
            sr.small_rollout_ensemble_reduce(self.ens, self.slab, sr.slab_rows_written(B, width), row, self.grad.shape[1], self.grad,
                                             self.rewards, n_el, ignore_periods * ld, self.totals, self.scratch)
        else:   # the same reduction, costs only: an evaluation pass returns the very bits a training pass does
            sr.small_rollout_ensemble_reduce(self.ens, None, 0, 0, 0, None, self.rewards, n_el, ignore_periods * ld, self.totals,
                                             self.scratch)
        self._note("reduce")
        tt = self.totals.clone()   # (the caller's tensors must not change under a later step)
        if train:
            sr.assign_grads(self.param_grads(), accumulate_grads)
        return tt[:, 0], tt[:, 1]
