"""K small policies in one launch pair (nic_small_rollout_ensemble_*, SmallPolicyEnsemble) on a real MI355X.

Every model of an ensemble launch runs the single-model kernels' instruction stream on its own slice of the buffers, so the bar
is BIT equality with K single-model launches (`nic_small_rollout_fwd` / `_bwd_wgrad` / `_reduce`, `FusedRollout.run`), with
strides longer than the slices and NaN in every gap; one slot is also held to the reference's golden vectors."""
import copy
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

from golden_io import Golden
from neural_inventory_control_amd import _lib, small_rollout as sr, workloads
from neural_inventory_control_amd.data_handling import Scenario
from neural_inventory_control_amd.layout import EnvProblem, Table, to_soa
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.policy_layers import materialize_linears
from neural_inventory_control_amd.rollout import FusedRollout
from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
from small_rollout_checks import SMALL_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PAD = dict(weights=5, rewards=8, final_state=4, states=8, hidden=12, logits=4, slab=8, grad=4, scratch=4)   # floats past a slice
ROW_PAD = 3   # floats past the packed weights in a slab row


def _bits(a, b):
    """bit equality (NaN-filled regions that nobody wrote compare equal too)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- launch level ------------------------------------------------------------------------------------------------------------------
class _Setting:
    """what a launch needs besides the weights: the problem tables, the demand trace and the initial state"""

    def __init__(self, prob, head, dims, data, T, ub, n_stores):
        self.prob, self.head, self.dims, self.T, self.ub, self.n_stores = prob, head, dims, T, ub, n_stores
        self.plan = sr.SmallRolloutPlan(prob, head, dims)
        B, ld = prob.B, prob.ldb
        self.demand = torch.zeros(data["demands"].shape[2], 1, ld, device=DEV)
        self.demand[:, :, :B] = data["demands"].permute(2, 1, 0)
        parts = [to_soa(data["initial_inventories"], ld).reshape(-1, ld)]
        if head != "softplus":
            if prob.Wn:
                parts.append(to_soa(data["initial_warehouse_inventories"], ld).reshape(-1, ld))
            if prob.E:
                parts.append(to_soa(data["initial_echelon_inventories"], ld).reshape(-1, ld))
        self.state0 = torch.cat(parts).contiguous()
        self.P0 = sr.packed_weight_count(self.plan.F, self.plan.n_hidden, self.plan.n_out)
        self.g_reward = torch.zeros(ld, device=DEV)
        self.g_reward[:B] = 1.0 / (B * T * n_stores)

    def desc(self, weights, width, round_orders=False):
        return self.plan.desc(self.T, 0, weights, self.demand, self.state0, self.ub, round_orders=round_orders, prob=self.prob,
                              lane_scenarios=width)


@functools.lru_cache(maxsize=None)
def _golden_setting(name):
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    prob = EnvProblem(c["problem_params"], data, DEV)
    head = "softplus" if c["policy"] == "vanilla_one_store" else "serial"
    idx = sorted({int(k.split(".")[2]) for k in g.params})
    packed = torch.cat([t.reshape(-1) for i in idx for t in (g.params[f"net.master.{i}.weight"], g.params[f"net.master.{i}.bias"])]).to(DEV)
    dims = [g.params[f"net.master.{idx[0]}.weight"].shape[1]] + [g.params[f"net.master.{i}.weight"].shape[0] for i in idx]
    assert sr.SmallRolloutPlan.supports(prob, head, dims)
    s = _Setting(prob, head, dims, data, c["periods"], float(g.z["warehouse_upper_bound"][0]), c["problem_params"]["n_stores"])
    return s, packed, g, idx


@functools.lru_cache(maxsize=None)
def _synthetic_data(chain, B, T):
    """chains that take the run-time-structure instantiations (SHAPE 0): one store with a 3-slot pipeline; store + warehouse + ONE
    echelon - and the two chains that are compiled in, as the workloads have them: "one_store" (cfg2), "serial" (cfg4)"""
    setting, policy, _, _, _ = workloads.get("cfg2" if chain.startswith("one_store") else "cfg4")
    setting = copy.deepcopy(setting)
    if chain == "one_store_ws3":
        setting["store_params"]["lead_time"] = {"sample_across_stores": False, "vary_across_samples": False, "expand": True, "value": 3}
        setting["store_params"]["initial_inventory"]["inventory_periods"] = 3
    elif chain == "serial_one_echelon":
        setting["problem_params"]["n_extra_echelons"] = 1
        setting["echelon_params"] = {"holding_cost": [0.1], "lead_time": [3]}
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], B, obs,
                  setting["seeds"])
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    return setting, data


def _synthetic_setting(chain, n_hidden, B, T):
    setting, data = _synthetic_data(chain, B, T)
    prob = EnvProblem(setting["problem_params"], data, DEV)
    if chain.startswith("one_store"):
        head, F, n_out = "softplus", prob.Ws, 1
        assert (prob.Ws, prob.Wn, prob.E) == (3 if chain == "one_store_ws3" else 4, 0, 0)
    else:
        head, F, n_out = "serial", prob.Ws + prob.Ww + prob.E * prob.We, prob.E + 2
        assert (prob.Wn, prob.E) == (1, 1 if chain == "serial_one_echelon" else 2)
    dims = [F] + [32] * n_hidden + [n_out]
    assert sr.SmallRolloutPlan.supports(prob, head, dims)
    return _Setting(prob, head, dims, data, T, 37.0, setting["problem_params"]["n_stores"])


def _random_packed(s, K, seed):
    """K packed weight vectors of PyTorch's default Linear scale (uniform +-1/sqrt(fan_in))"""
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(K):
        parts = []
        for _, n, k, _ in sr.layer_slices(s.plan.F, s.plan.n_hidden, s.plan.n_out):
            bound = 1.0 / np.sqrt(k)
            parts += [(torch.rand(n * k, generator=gen) * 2 - 1) * bound, (torch.rand(n, generator=gen) * 2 - 1) * bound]
        rows.append(torch.cat(parts))
    return torch.stack(rows).to(DEV)


def _padded(K, slice_, stride, fill=NAN, inside=None):
    """[K][stride] filled with `fill`; `inside`: value of the first slice_ floats of every row (None: `fill` too)"""
    t = torch.full((K, stride), fill, device=DEV)
    if inside is not None:
        t[:, :slice_] = inside
    return t


def _run_ensemble(s, packed, width, train=True, round_orders=False):
    """ensemble forward (+ backward + reduce) with every stride longer than its slice and NaN in the gaps -> the buffers [K][stride],
    the slices and the kernel names"""
    K = packed.shape[0]
    w = _padded(K, s.P0, s.P0 + PAD["weights"])
    w[:, :s.P0] = packed
    d = s.desc(w, width, round_orders)
    sl = sr.ensemble_slices(d)
    assert sl["weights"] == s.P0
    st = {k: sl[k] + PAD[k] for k in ("weights", "rewards", "final_state", "states", "hidden", "logits")}
    row = s.P0 + ROW_PAD
    st["slab"] = sl["slab_rows"] * row + PAD["slab"]
    st["grad"] = s.P0 + PAD["grad"]
    st["scratch"] = sr.small_rollout_reduce_scratch(sl["slab_rows"], s.P0, sl["rewards"]) + PAD["scratch"]
    ens = sr.ensemble_strides(K, **st)
    # (the padding columns [B, ldb) of the costs are summed by the reduction: a slice starts as zeros, like the single-model buffer)
    buf = dict(weights=w, rewards=_padded(K, sl["rewards"], st["rewards"], inside=0.0), final_state=_padded(K, 0, st["final_state"]),
               totals=torch.full((K, 2), NAN, device=DEV), scratch=_padded(K, 0, st["scratch"]))
    names = {}
    if train:
        for k in ("states", "hidden", "logits", "slab", "grad"):
            buf[k] = _padded(K, 0, st[k])
    hist = (buf["states"], buf["hidden"], buf["logits"]) if train else (None, None, None)
    sr.small_rollout_ensemble_fwd(d, ens, buf["rewards"], buf["final_state"], *hist)
    names["fwd"] = _lib.lib().nic_last_kernel().decode()
    n_el, ign = sl["rewards"], (s.T // 2) * s.prob.ldb
    if train:
        sr.small_rollout_ensemble_bwd_wgrad(d, ens, *hist, Table(s.g_reward, 0, 1), buf["slab"], row)
        names["bwd"] = _lib.lib().nic_last_kernel().decode()
        sr.small_rollout_ensemble_reduce(ens, buf["slab"], sl["slab_rows"], row, s.P0, buf["grad"], buf["rewards"], n_el, ign, buf["totals"],
                                         buf["scratch"])
    else:
        sr.small_rollout_ensemble_reduce(ens, None, 0, 0, 0, None, buf["rewards"], n_el, ign, buf["totals"], buf["scratch"])
    names["reduce"] = _lib.lib().nic_last_kernel().decode()
    torch.cuda.synchronize()
    return buf, sl, st, row, names


def _run_single(s, packed_row, width, sl, row, train=True, round_orders=False):
    """the single-model entry points on one model's weights; buffers of exactly one slice, initialised like the ensemble's"""
    w = packed_row.clone()
    d = s.desc(w, width, round_orders)
    one = lambda n, v=NAN: torch.full((n,), v, device=DEV)  # noqa: E731
    buf = dict(rewards=one(sl["rewards"], 0.0), final_state=one(sl["final_state"]), totals=one(2))
    if train:
        buf.update(states=one(sl["states"]), hidden=one(sl["hidden"]), logits=one(sl["logits"]), slab=one(sl["slab_rows"] * row),
                   grad=one(s.P0))
    hist = (buf["states"], buf["hidden"], buf["logits"]) if train else (None, None, None)
    sr.small_rollout_fwd(d, buf["rewards"], buf["final_state"], *hist)
    rewards2d = buf["rewards"].view(s.T, s.prob.ldb)
    scratch = torch.empty(sr.small_rollout_reduce_scratch(sl["slab_rows"], s.P0, sl["rewards"]), device=DEV)
    if train:
        slab2d = buf["slab"].view(sl["slab_rows"], row)
        sr.small_rollout_bwd_wgrad(d, *hist, Table(s.g_reward, 0, 1), slab2d)
        sr.small_rollout_reduce(slab2d, sl["slab_rows"], buf["grad"], rewards2d, s.T // 2, buf["totals"], scratch)
    else:
        sr.small_rollout_reduce(None, 0, None, rewards2d, s.T // 2, buf["totals"], scratch)
    torch.cuda.synchronize()
    return buf


def _compare_with_single_launches(s, packed, width, train=True, round_orders=False, kernels=None):
    """kernels: {"fwd": ..., "bwd": ...} the recorded names the launches must have (None: only their `models=K`)"""
    K, B = packed.shape[0], s.prob.B
    buf, sl, st, row, names = _run_ensemble(s, packed, width, train, round_orders)
    for tag, name in names.items():
        assert f"models={K}" in name, (tag, name)
    if kernels is not None:
        assert {tag: names[tag] for tag in kernels} == kernels
    assert ("small_rollout16" in names["fwd"]) == (width == 16)
    size = dict(sl, slab=sl["slab_rows"] * row, grad=s.P0, scratch=0)
    keys = ("rewards", "final_state") + (("states", "hidden", "logits", "slab", "grad") if train else ())
    for m in range(K):
        one = _run_single(s, packed[m], width, sl, row, train, round_orders)
        for k in keys:
            assert _bits(buf[k][m, :size[k]], one[k]), (k, m)
        assert _bits(buf["totals"][m], one["totals"]), m
    # nothing wrote into a gap (the scratch's own slice is the kernels' to use), nothing read one: the live results are finite
    for k in keys + ("weights", "scratch"):
        assert bool(torch.isnan(buf[k][:, size[k] if k != "scratch" else st[k] - PAD[k]:]).all()), k
    T, ld, F = s.T, s.prob.ldb, s.plan.F
    assert bool(torch.isfinite(buf["rewards"][:, :sl["rewards"]].view(K, T, ld)[:, :, :B]).all())
    assert bool(torch.isfinite(buf["final_state"][:, :sl["final_state"]].view(K, F, ld)[:, :, :B]).all())
    assert bool(torch.isnan(buf["final_state"][:, :sl["final_state"]].view(K, F, ld)[:, :, B:]).all())   # columns past the live ones
    assert bool(torch.isfinite(buf["totals"]).all())
    if train:
        assert bool(torch.isfinite(buf["grad"][:, :s.P0]).all())
        slab = buf["slab"][:, :size["slab"]].view(K, sl["slab_rows"], row)
        assert bool(torch.isfinite(slab[:, :, :s.P0]).all()) and bool(torch.isnan(slab[:, :, s.P0:]).all())
    return buf, sl


def _perturbed(packed, K, seed, keep=None):
    gen = torch.Generator().manual_seed(seed)
    out = torch.stack([packed.cpu() + 0.02 * torch.randn(packed.numel(), generator=gen) * packed.cpu().abs().mean() for _ in range(K)])
    if keep is not None:
        out[keep] = packed.cpu()
    return out.to(DEV)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_ensemble_launches_equal_single_launches_on_the_fixtures(name, width, K):
    s, packed, _, _ = _golden_setting(name)
    _compare_with_single_launches(s, _perturbed(packed, K, 11), width)


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("B", [16, 40, 100])
@pytest.mark.parametrize("n_hidden", [1, 2, 3])
@pytest.mark.parametrize("chain", ["one_store_ws3", "serial_one_echelon"])
def test_ensemble_launches_equal_single_launches_on_run_time_structure_chains(chain, n_hidden, B, width):
    """the SHAPE 0 instantiations: ragged last wavefronts at both widths, one period and several, 2 and 5 models"""
    for T, K in ((1, 2), (7, 5), (1, 5), (7, 2)):
        s = _synthetic_setting(chain, n_hidden, B, T)
        _compare_with_single_launches(s, _random_packed(s, K, 1000 * T + K), width)


# the compiled-in chains at the depths the fixtures lack (cfg2's policy has three hidden layers, cfg4's two): recorded names, literally
COMPILED_IN_KERNELS = {
    ("one_store", 2, 16): {"fwd": "small_rollout16_fwd_kernel<2,one_store,models=3>", "bwd": "small_rollout16_bwd_kernel<2,wgrad,one_store,models=3>"},
    ("one_store", 2, 32): {"fwd": "small_rollout_fwd_mfma_kernel<2,one_store,models=3>",
                           "bwd": "small_rollout_bwd_mfma_kernel<2,wgrad,one_store,models=3>"},
    ("serial", 3, 16): {"fwd": "small_rollout16_fwd_kernel<3,serial,models=3>", "bwd": "small_rollout16_bwd_kernel<3,wgrad,serial,models=3>"},
    ("serial", 3, 32): {"fwd": "small_rollout_fwd_mfma_kernel<3,serial,models=3>", "bwd": "small_rollout_bwd_mfma_kernel<3,wgrad,serial,models=3>"},
}


@pytest.mark.parametrize("chain,n_hidden,width", sorted(COMPILED_IN_KERNELS))
def test_ensemble_launches_equal_single_launches_on_the_compiled_in_chains_at_the_other_depths(chain, n_hidden, width):
    """<2,one_store> and <3,serial>: 40 scenarios (three 16-scenario wavefronts or two 32-scenario ones, the last ragged), 5 periods"""
    s = _synthetic_setting(chain, n_hidden, 40, 5)
    assert tuple(s.dims) == ((4, 32, 32, 1) if chain == "one_store" else (15, 32, 32, 32, 4))
    kernels = COMPILED_IN_KERNELS[chain, n_hidden, width]
    assert all(k.endswith(",models=3>") for k in kernels.values())
    _compare_with_single_launches(s, _random_packed(s, 3, 77), width, kernels=kernels)


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_ensemble_evaluation_without_histories_and_with_rounded_orders(name, width):
    s, packed, _, _ = _golden_setting(name)
    _compare_with_single_launches(s, _perturbed(packed, 3, 12), width, train=False, round_orders=True)


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("name", SMALL_CASES)
def test_one_slot_of_an_ensemble_meets_the_golden_vectors(name, width):
    """K = 3 with the fixture's parameters in slot 1: that slot's rewards, per-scenario totals and gradients (from the reduced
    [K][P] buffer) at the bars of tests/small_rollout_checks.py"""
    s, packed, g, idx = _golden_setting(name)
    buf, sl, _, _, _ = _run_ensemble(s, _perturbed(packed, 3, 13, keep=1), width)
    T, B, ld = s.T, s.prob.B, s.prob.ldb
    rewards = buf["rewards"][1, :sl["rewards"]].view(T, ld)
    ref_r = g.tensor("rewards")
    torch.testing.assert_close(rewards[:, :B].cpu(), ref_r, rtol=1e-5, atol=1e-4)
    tot_b, ref_b = rewards[:, :B].double().sum(dim=0).cpu(), ref_r.double().sum(dim=0)
    assert float(((tot_b - ref_b).abs() / ref_b.abs().clamp_min(1e-9)).max()) <= 1e-5
    assert float(rewards[:, B:].abs().sum()) == 0.0
    grad = buf["grad"][1, :s.P0].double().cpu()
    for (o, n, k, bo), i in zip(sr.layer_slices(s.plan.F, s.plan.n_hidden, s.plan.n_out), idx):
        for got, key in ((grad[o:o + n * k].view(n, k), f"net.master.{i}.weight"), (grad[bo:bo + n], f"net.master.{i}.bias")):
            ref = g.grads[key].double()
            rel = float((got - ref).norm() / (ref.norm() + 1e-30))
            assert rel <= 1e-5, (key, rel)


# ---- engine level ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _workload(workload, B, T):
    setting, policy, _, _, _ = workloads.get(workload)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], B, obs,
                  setting["seeds"])
    return setting, policy, obs, sc, {k: v.to(DEV) for k, v in sc.get_data().items()}


def _fresh_models(workload, B, T, seeds):
    setting, policy, obs, sc, data = _workload(workload, B, T)
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if policy["name"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories") if k in data)
    models = []
    for seed in seeds:
        torch.manual_seed(seed)
        m = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        materialize_linears(m.master_linears(), F)
        models.append(m)
    return models


def _clones(models):
    out = copy.deepcopy(models)
    for m in out:
        for p in m.parameters():
            p.grad = None
    return out


def _grads(models):
    return [[p.grad.clone() for p in m.parameters()] for m in models]


def _same_grads(a, b):
    return all(torch.equal(x, y) for ga, gb in zip(a, b) for x, y in zip(ga, gb))


@pytest.mark.parametrize("workload,policy_name", [("cfg1", "vanilla_one_store"), ("cfg4", "vanilla_serial")])
def test_engine_equals_k_single_model_engines(workload, policy_name):
    B, T, K, ign = 96, 8, 3, 2
    setting, policy, obs, _, data = _workload(workload, B, T)
    assert policy["name"] == policy_name
    models = _fresh_models(workload, B, T, (1, 2, 3))
    alone = _clones(models)
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    singles = [FusedRollout(m, setting["problem_params"], DEV) for m in alone]

    def both(data, train, accumulate=False, discrete=False):
        tot, rep = ens.run(data, T, ign, train=train, observation_params=obs, accumulate_grads=accumulate, discrete_allocation=discrete)
        assert tuple(tot.shape) == tuple(rep.shape) == (K,)
        for m, eng in enumerate(singles):
            t1, r1 = eng.run(data, T, ign, train=train, observation_params=obs, accumulate_grads=accumulate, discrete_allocation=discrete)
            assert torch.equal(tot[m], t1) and torch.equal(rep[m], r1), (m, float(tot[m]), float(t1))
            assert torch.equal(ens.rewards[m], eng.rewards)
        torch.cuda.synchronize()

    both(data, True)
    assert _same_grads(_grads(models), _grads(alone))
    assert "models=3" in ens.last_kernels["fwd"] and "models=3" in ens.last_kernels["bwd"] and "models=3" in ens.last_kernels["reduce"]
    # the gradients are views into ONE [K][P] buffer
    base = ens.grad.data_ptr()
    assert all(base <= p.grad.data_ptr() < base + ens.grad.numel() * 4 for m in models for p in m.parameters())
    kept = {k: getattr(ens, k).data_ptr() for k in ("weights", "rewards", "states", "hidden", "logits", "slab", "grad", "scratch")}
    both(data, False)
    both(data, False, discrete=True)
    # buffers are allocated once per (B, T, K): evaluation runs in between keep the training buffers
    assert kept == {k: getattr(ens, k).data_ptr() for k in kept}
    # accumulate over two calls: the first call's gradients are the engine's views, so they are cloned as a training loop would not
    # have to - param.grad of a fresh optimizer step is a tensor of its own
    for ms in (models, alone):
        for m in ms:
            for p in m.parameters():
                p.grad = torch.ones_like(p)
    both(data, True, accumulate=True)
    both(data, True, accumulate=True)
    assert kept == {k: getattr(ens, k).data_ptr() for k in kept}
    assert _same_grads(_grads(models), _grads(alone))
    assert all(p.grad.data_ptr() < base or p.grad.data_ptr() >= base + ens.grad.numel() * 4 for m in models for p in m.parameters())
    # the parameters changed: the weights are packed again
    with torch.no_grad():
        for ms in (models, alone):
            for i, m in enumerate(ms):
                for p in m.parameters():
                    p.mul_(1.0 + 0.05 * (i + 1))
                    p.grad = None
    both(data, True)
    assert _same_grads(_grads(models), _grads(alone))
    # a shorter last batch through the same engines
    _, _, _, _, short = _workload(workload, 40, T)
    both(short, True)
    assert _same_grads(_grads(models), _grads(alone))


def test_three_models_train_independently():
    """three seeds, three Adam optimizers at three learning rates, five steps: the ensemble's parameters end where each model's own
    FusedRollout loop ends"""
    B, T = 128, 8
    setting, policy, obs, _, pool = _workload("cfg1", 5 * B, T)
    models = _fresh_models("cfg1", 5 * B, T, (21, 22, 23))
    alone = _clones(models)
    lrs = (1e-2, 3e-3, 1e-3)
    batches = [{k: v[i * B:(i + 1) * B] for k, v in pool.items()} for i in range(5)]   # (five batches of B scenarios)
    assert all(v.shape[0] == 5 * B for v in pool.values()) and not torch.equal(batches[0]["demands"], batches[1]["demands"])
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(models, lrs)]
    for data in batches:
        ens.run(data, T, 2, train=True, observation_params=obs)
        for opt in opts:
            opt.step()
    for m, lr in zip(alone, lrs):
        eng, opt = FusedRollout(m, setting["problem_params"], DEV), torch.optim.Adam(m.parameters(), lr=lr)
        for data in batches:
            eng.run(data, T, 2, train=True, observation_params=obs)
            opt.step()
    torch.cuda.synchronize()
    for a, b in zip(models, alone):
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)
    assert not torch.equal(next(models[0].parameters()), next(models[1].parameters()))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_mismatched_and_unsupported_models():
    setting, policy, obs, sc, data = _workload("cfg1", 96, 8)
    good = _fresh_models("cfg1", 96, 8, (1,))
    narrow = copy.deepcopy(policy)
    narrow["neurons_per_hidden_layer"]["master"] = policy["neurons_per_hidden_layer"]["master"][:-1]
    other = NeuralNetworkCreator().create_neural_network(sc, narrow, device=DEV)
    with pytest.raises(ValueError, match="model 1: architecture"):
        SmallPolicyEnsemble(good + [other], setting["problem_params"], DEV)
    s3, p3, _, sc3, _ = _workload("cfg3", 64, 4)
    with pytest.raises(ValueError, match="model 0"):
        SmallPolicyEnsemble([NeuralNetworkCreator().create_neural_network(sc3, p3, device=DEV)], s3["problem_params"], DEV)
    ens = SmallPolicyEnsemble(good, setting["problem_params"], DEV)
    with pytest.raises(ValueError, match="discrete_allocation"):
        ens.run(data, 8, 0, train=True, observation_params=obs, discrete_allocation=True)


@pytest.mark.parametrize("what", ["no_models", "short_rewards_stride", "short_states_stride", "short_slab_row", "short_grad_stride"])
def test_refused_requests_launch_nothing(what):
    """non-zero status, a message, and the poisoned outputs unchanged"""
    s, packed, _, _ = _golden_setting("cfg1_one_store_lost_vanilla")
    K, width = 2, 16
    w = _perturbed(packed, K, 14)
    d = s.desc(w, width)
    sl = sr.ensemble_slices(d)
    row = sl["slab_row_stride"]
    st = {k: sl[k] for k in ("weights", "rewards", "final_state", "states", "hidden", "logits", "slab", "grad", "scratch")}
    n_models = K
    if what == "no_models":
        n_models = 0
    elif what == "short_rewards_stride":
        st["rewards"] -= 4
    elif what == "short_states_stride":
        st["states"] -= 4
    elif what == "short_slab_row":
        row = s.P0 - 1
    elif what == "short_grad_stride":
        st["grad"] = s.P0 - 1
    ens = sr.ensemble_strides(n_models, **st)
    POISON = -12345.0
    buf = {k: torch.full((K, sl[k]), POISON, device=DEV) for k in ("rewards", "final_state", "states", "hidden", "logits", "slab", "grad", "scratch")}
    totals = torch.full((K, 2), POISON, device=DEV)
    lib = _lib.lib()
    stream = _lib.current_stream()
    hist = [buf[k].data_ptr() for k in ("states", "hidden", "logits")]
    calls = {
        "fwd": lambda: lib.nic_small_rollout_ensemble_fwd(d, ens, buf["rewards"].data_ptr(), buf["final_state"].data_ptr(), *hist, stream),
        "bwd": lambda: lib.nic_small_rollout_ensemble_bwd_wgrad(d, ens, *hist, Table(s.g_reward, 0, 1).t2(), buf["slab"].data_ptr(), row,
                                                                stream),
        "reduce": lambda: lib.nic_small_rollout_ensemble_reduce(ens, buf["slab"].data_ptr(), sl["slab_rows"], row, s.P0,
                                                                buf["grad"].data_ptr(), buf["rewards"].data_ptr(), sl["rewards"], 0,
                                                                totals.data_ptr(), buf["scratch"].data_ptr(), stream)}
    # only the calls the request is refused by are made: nothing runs on the poisoned buffers
    refused = {"no_models": ("fwd", "bwd", "reduce"), "short_rewards_stride": ("fwd", "reduce"), "short_states_stride": ("fwd", "bwd"),
               "short_slab_row": ("bwd", "reduce"), "short_grad_stride": ("reduce",)}[what]
    for call in refused:
        assert calls[call]() != 0, call
        message = lib.nic_last_error().decode()
        assert message.startswith("nic_small_rollout_ensemble_" + ("bwd_wgrad" if call == "bwd" else call) + ":"), message
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool((t == POISON).all()), k
    assert bool((totals == POISON).all())
