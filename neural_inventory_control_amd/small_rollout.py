"""Whole-horizon rollout of the small (32-wide, one-store chain) policies through `nic_small_rollout_*` (csrc/small_rollout.hip:
32 scenarios per wavefront, csrc/small_rollout16.hip: 16): ONE kernel runs all T periods of `Trainer.simulate_batch`
(trainer.py:190-213) with the layers on the matrix cores, the weights resident in registers and the per-scenario state, head and env
step per lane; a second kernel sweeps the horizon backwards and contracts the weight gradients itself (one partial gradient per
wavefront), and `nic_small_rollout_reduce` sums those and the costs.  `nic_small_rollout_bwd`, the backward sweep that writes a dz
history for one weight-gradient GEMM per layer, is kept as the referee of the in-kernel gradients.  Which kernel instantiation a
request runs is decided in csrc/small_rollout_variants.h.  Used by `FusedRollout` when `SmallRolloutPlan.supports(...)` and by
`SmallPolicyEnsemble` (K models in one launch pair, on one batch or on I problem instances); the rules both engines follow around the launches (`lane_width`, `slab_rows_written`, `set_g_reward`,
`assign_grads`) are here.

Descriptor building is pointer plumbing and device-agnostic (the CPU test build of the kernel bodies uses it too).
"""
import torch

from . import _lib, ops
from ._lib import NicSmallRolloutDesc, NicTable2
from .layout import EnvProblem, Table

HEAD_SOFTPLUS, HEAD_SERIAL = 0, 1
H = _lib.NIC_SR_HIDDEN


def packed_weight_count(F, n_hidden, n_out):
    return (H * F + H) + (n_hidden - 1) * (H * H + H) + (n_out * H + n_out)


def pack_weights(linears, out=None):
    """[W1 (32 x F), b1] [W_l (32 x 32), b_l]... [Wout (n_out x 32), bout] as one flat float32 tensor."""
    parts = []
    for m in linears:
        parts += [m.weight.detach().reshape(-1), m.bias.detach().reshape(-1)]
    if out is None:
        return torch.cat(parts).contiguous()
    if out.numel() != sum(p.numel() for p in parts):   # (torch.cat would silently re-allocate `out`: kernels hold its address)
        raise ValueError("pack_weights: the output buffer does not have packed_weight_count elements")
    torch.cat(parts, out=out)   # (one launch)
    return out


def layer_slices(F, n_hidden, n_out):
    """[(weight offset, rows, cols, bias offset)] per layer in the packed buffer."""
    out, off, k = [], 0, F
    for i in range(n_hidden + 1):
        n = H if i < n_hidden else n_out
        out.append((off, n, k, off + n * k))
        off += n * k + n
        k = n
    return out


class SmallRolloutPlan:
    """Shapes of one small-policy rollout; `supports` says whether the fused kernels apply."""

    def __init__(self, prob: EnvProblem, head, dims):
        self.prob, self.head, self.dims = prob, head, list(dims)
        self.F = prob.Ws + prob.Wn * prob.Ww + prob.E * prob.We
        self.n_hidden = len(dims) - 2
        self.n_out = dims[-1]

    @staticmethod
    def supports(prob: EnvProblem, head, dims):
        F = prob.Ws + prob.Wn * prob.Ww + prob.E * prob.We
        n_hidden = len(dims) - 2
        return (head in ("softplus", "serial") and prob.S == 1 and prob.Wn <= 1 and prob.E <= 3
                and (prob.Wn == 1 or prob.E == 0) and F <= _lib.NIC_SR_MAX_INPUTS and dims[0] == F
                and 1 <= n_hidden <= 3 and all(w == H for w in dims[1:-1]) and dims[-1] <= _lib.NIC_SR_MAX_OUTPUTS
                and (head != "softplus" or dims[-1] == 1) and (head != "serial" or dims[-1] == prob.E + 2))

    def desc(self, T, t0, weights, demand_soa, state0, upper_bound, round_orders=False, prob=None, lane_scenarios=0):
        """demand_soa: [T_total][1][ldb]; state0: [F][ldb]; prob: the CURRENT batch's EnvProblem (same shapes as the
        plan's; its cost / lead-time tables are the ones the kernels read)."""
        p = prob if prob is not None else self.prob
        d = NicSmallRolloutDesc()
        d.n_scenarios, d.ldb, d.T, d.t0 = p.B, p.ldb, T, t0
        d.F, d.n_hidden, d.n_out = self.F, self.n_hidden, self.n_out
        d.head = HEAD_SERIAL if self.head == "serial" else HEAD_SOFTPLUS
        d.Ws, d.Wn, d.Ww, d.E, d.We = p.Ws, p.Wn, p.Ww, p.E, p.We
        d.lost_demand, d.maximize_profit = int(p.lost_demand), int(p.maximize_profit)
        d.detach_input = int(self.head == "serial")
        d.round_orders = int(bool(round_orders))
        d.upper_bound = float(upper_bound)
        d.lane_scenarios = int(lane_scenarios)   # 16 or 32 scenarios per wavefront; 0 means 32 (the engines choose with `lane_width`)
        d.weights, d.demand, d.state0 = weights.data_ptr(), demand_soa.data_ptr(), state0.data_ptr()
        d.underage, d.holding = p.underage.t2(), p.holding.t2()
        lead = p.lead  # (s, w, b) table with one store and one supplier column
        d.lead = NicTable2(_lib.ptr(lead.tensor), lead.loc_stride, lead.scn_stride)
        d.wh_holding, d.wh_lead, d.wh_edge = p.wh_holding.t2(), p.wh_lead.t2(), p.wh_edge.t2()
        d.ech_holding, d.ech_lead = p.ech_holding.t2(), p.ech_lead.t2()
        self._keep = (weights, demand_soa, state0, p)
        return d


def lane_width(requested, train, B):
    """Scenarios per wavefront of a run: `requested` (16 or 32) if set.  Training: 16 (v_mfma_f32_16x16x4_f32, wave-native
    activation history) - measured against 32: cfg1 0.55 -> 0.30 ms, cfg4 (16,384 scenarios: 32 leaves half the SIMDs without a
    wavefront) 0.83 -> 0.70 ms, cfg2 (32,768) 1.16 -> 1.07 ms, 65,536 scenarios 2.28 -> 1.87 ms.  Evaluation (no history): 16
    while 32 would leave SIMDs idle, else 32 (the per-lane head / env-step code is replicated in four lane groups instead of two)."""
    return requested or (16 if (train or B <= 16384) else 32)


def slab_rows_written(B, width):
    """Rows of the partial-gradient slab a backward launch of this width wrote: one per wavefront.  The slab is sized for the 16-wide
    form; a 32-wide launch fills half of it, and the reduction must not pick up an earlier 16-wide run's rows."""
    return (B + width - 1) // width


def set_g_reward(g_reward, B, grad_scale, last_key):
    """g_reward[b] = d loss / d reward[b, t] for the live scenarios, 0 in the padding columns.  Two launches that a training loop
    repeats with the same numbers every step: skipped while the buffer, the batch size and the (host-side) scale are those of
    `last_key`, the key the previous call returned (None: fill).  Returns the key of this call."""
    key = (g_reward.data_ptr(), B, grad_scale) if isinstance(grad_scale, (int, float)) else None
    if key is None or key != last_key:
        g_reward.zero_()
        g_reward[:B] = grad_scale
    return key


def assign_grads(param_grads, accumulate):
    """param.grad <- the engine's gradient buffer; `accumulate` adds to a gradient that is already there (unless that IS the
    engine's buffer from an earlier run, which this run has overwritten)."""
    for p, g in param_grads:
        if accumulate and p.grad is not None and p.grad is not g:
            p.grad.add_(g)
        else:
            p.grad = g


def small_rollout_fwd(desc, rewards, state_final, states_hist, hidden_hist, logits_hist):
    ops._dev(rewards)
    _lib.check(_lib.lib().nic_small_rollout_fwd(desc, _lib.ptr(rewards), _lib.ptr(state_final), _lib.ptr(states_hist),
                                                _lib.ptr(hidden_hist), _lib.ptr(logits_hist), _lib.current_stream()))


def small_rollout_bwd(desc, states_hist, hidden_hist, logits_hist, g_reward: Table, dz_hidden, dz_out):
    ops._dev(dz_out)
    _lib.check(_lib.lib().nic_small_rollout_bwd(desc, _lib.ptr(states_hist), _lib.ptr(hidden_hist), _lib.ptr(logits_hist),
                                                g_reward.t2(), _lib.ptr(dz_hidden), _lib.ptr(dz_out),
                                                _lib.current_stream()))


def small_rollout_bwd_wgrad_slots(n_scenarios):
    return _lib.lib().nic_small_rollout_bwd_wgrad_slots(int(n_scenarios))


def small_rollout_bwd_wgrad(desc, states_hist, hidden_hist, logits_hist, g_reward: Table, slab):
    """Backward sweep with in-kernel weight gradients: slab [slots][>= packed_weight_count] receives one partial gradient per
    wavefront in the packed-weight layout (sum over dim 0 = d total / d packed weights)."""
    ops._dev(slab)
    _lib.check(_lib.lib().nic_small_rollout_bwd_wgrad(desc, _lib.ptr(states_hist), _lib.ptr(hidden_hist), _lib.ptr(logits_hist),
                                                      g_reward.t2(), _lib.ptr(slab), slab.stride(0), _lib.current_stream()))


def small_rollout_reduce_scratch(n_rows, P, n_reward_elems):
    return int(_lib.lib().nic_small_rollout_reduce_scratch(int(n_rows), int(P), int(n_reward_elems)))


def small_rollout_reduce(slab, n_rows, grad, rewards, ignore_periods, totals, scratch):
    """grad <- sum of the first n_rows rows of slab; totals <- [sum of rewards [T][ldb], sum of its periods >= ignore_periods]:
    two launches with a fixed summation order (csrc/small_reduce.hip).  Either pair may be None."""
    ops._dev(scratch)
    P = grad.numel() if grad is not None else 0
    n_el = rewards.numel() if rewards is not None else 0
    assert scratch.numel() >= small_rollout_reduce_scratch(n_rows if slab is not None else 0, P, n_el)
    assert rewards is None or rewards.is_contiguous()
    _lib.check(_lib.lib().nic_small_rollout_reduce(_lib.ptr(slab), int(n_rows), slab.stride(0) if slab is not None else 0, P,
                                                   _lib.ptr(grad), _lib.ptr(rewards), n_el,
                                                   int(ignore_periods) * rewards.shape[-1] if rewards is not None else 0,
                                                   _lib.ptr(totals), _lib.ptr(scratch), _lib.current_stream()))


# ---- K models of one architecture on one batch (nic_small_rollout_ensemble_*, csrc/small_ensemble_plan.h) ----------------------------
SLICE_FIELDS = tuple(n for n, _ in _lib.NicSmallEnsembleSlices._fields_)
STRIDE_FIELDS = tuple(n for n, _ in _lib.NicSmallEnsemble._fields_[2:])


def ensemble_slices(desc):
    """{buffer: floats of ONE model's slice} for a descriptor (its lane_scenarios decides the history rows) - the numbers the entry
    points check the strides against, from csrc/small_ensemble_plan.h.  Needs the library, not a device."""
    out = _lib.NicSmallEnsembleSlices()
    _lib.check(_lib.lib().nic_small_rollout_ensemble_slices(desc, out))
    return {n: int(getattr(out, n)) for n in SLICE_FIELDS}


def ensemble_strides(n_models, **strides):
    """NicSmallEnsemble: floats between two models' slices of every per-model buffer (buffers a call does not take: 0)."""
    e = _lib.NicSmallEnsemble()
    e.n_models = int(n_models)
    for k, v in strides.items():
        if k not in STRIDE_FIELDS:
            raise KeyError(k)
        setattr(e, k, int(v))
    return e


# `active` in the wrappers below: None launches the entry point as it always was; an int32 [K] device tensor (non-zero: the model runs)
# launches its `_active` twin, under which a model whose entry is zero has no byte of its slices read or written
def _mask(active, n_models):
    if not active.is_cuda or active.dtype != torch.int32 or tuple(active.shape) != (int(n_models),) or not active.is_contiguous():
        raise ValueError(f"the active mask must be a contiguous int32 [{int(n_models)}] device tensor, got {active.dtype} {tuple(active.shape)}")
    return _lib.ptr(active)


def small_rollout_ensemble_fwd(desc, ens, rewards, state_final, states_hist, hidden_hist, logits_hist, active=None):
    ops._dev(rewards)
    args = (desc, ens, _lib.ptr(rewards), _lib.ptr(state_final), _lib.ptr(states_hist), _lib.ptr(hidden_hist), _lib.ptr(logits_hist))
    if active is None:
        _lib.check(_lib.lib().nic_small_rollout_ensemble_fwd(*args, _lib.current_stream()))
    else:
        _lib.check(_lib.lib().nic_small_rollout_ensemble_fwd_active(*args, _mask(active, ens.n_models), _lib.current_stream()))


def small_rollout_ensemble_bwd_wgrad(desc, ens, states_hist, hidden_hist, logits_hist, g_reward: Table, slab, slab_row_stride, active=None):
    """slab [K][>= rows x slab_row_stride]: model m's wavefront w writes its partial gradient at m * ens.slab + w * slab_row_stride."""
    ops._dev(slab)
    args = (desc, ens, _lib.ptr(states_hist), _lib.ptr(hidden_hist), _lib.ptr(logits_hist), g_reward.t2(), _lib.ptr(slab), int(slab_row_stride))
    if active is None:
        _lib.check(_lib.lib().nic_small_rollout_ensemble_bwd_wgrad(*args, _lib.current_stream()))
    else:
        _lib.check(_lib.lib().nic_small_rollout_ensemble_bwd_wgrad_active(*args, _mask(active, ens.n_models), _lib.current_stream()))


def small_rollout_ensemble_reduce(ens, slab, n_rows, slab_row_stride, P, grad, rewards, n_reward_elems, ignore_elems, totals, scratch,
                                  active=None):
    """grad [K][ens.grad] <- column sums of every model's first n_rows slab rows; totals [K][2] <- every model's total / reported
    cost: `nic_small_rollout_reduce` for all K models in its two launches.  Either pair may be None."""
    ops._dev(scratch)
    args = (ens, _lib.ptr(slab), int(n_rows), int(slab_row_stride), int(P), _lib.ptr(grad), _lib.ptr(rewards), int(n_reward_elems),
            int(ignore_elems), _lib.ptr(totals), _lib.ptr(scratch))
    if active is None:
        _lib.check(_lib.lib().nic_small_rollout_ensemble_reduce(*args, _lib.current_stream()))
    else:
        _lib.check(_lib.lib().nic_small_rollout_ensemble_reduce_active(*args, _mask(active, ens.n_models), _lib.current_stream()))


# ---- K models on I problem instances (nic_small_rollout_instances_*, csrc/small_ensemble_plan.h) -------------------------------------
INSTANCE_FIELDS = tuple(n for n, _ in _lib.NicSmallInstances._fields_[2:])


def instance_strides(n_instances, **strides):
    """NicSmallInstances: floats between two instances' copies of the demand trace, the initial state and each of the eight tables
    (what is not named: 0, shared by all instances).  Model m of K runs on instance m // (K // n_instances)."""
    inst = _lib.NicSmallInstances()
    inst.n_instances = int(n_instances)
    for k, v in strides.items():
        if k not in INSTANCE_FIELDS:
            raise KeyError(k)
        setattr(inst, k, int(v))
    return inst


def small_rollout_instances_fwd(desc, ens, inst, rewards, state_final, states_hist, hidden_hist, logits_hist, active=None):
    """`small_rollout_ensemble_fwd` with every model on its instance's inputs; `desc` points at instance 0's."""
    ops._dev(rewards)
    args = (desc, ens, inst, _lib.ptr(rewards), _lib.ptr(state_final), _lib.ptr(states_hist), _lib.ptr(hidden_hist), _lib.ptr(logits_hist))
    if active is None:
        _lib.check(_lib.lib().nic_small_rollout_instances_fwd(*args, _lib.current_stream()))
    else:
        _lib.check(_lib.lib().nic_small_rollout_instances_fwd_active(*args, _mask(active, ens.n_models), _lib.current_stream()))


def small_rollout_instances_bwd_wgrad(desc, ens, inst, states_hist, hidden_hist, logits_hist, g_reward: Table, slab, slab_row_stride,
                                      active=None):
    ops._dev(slab)
    args = (desc, ens, inst, _lib.ptr(states_hist), _lib.ptr(hidden_hist), _lib.ptr(logits_hist), g_reward.t2(), _lib.ptr(slab),
            int(slab_row_stride))
    if active is None:
        _lib.check(_lib.lib().nic_small_rollout_instances_bwd_wgrad(*args, _lib.current_stream()))
    else:
        _lib.check(_lib.lib().nic_small_rollout_instances_bwd_wgrad_active(*args, _mask(active, ens.n_models), _lib.current_stream()))
