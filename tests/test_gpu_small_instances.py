"""K small policies on I problem instances in one launch pair (nic_small_rollout_instances_*, SmallPolicyEnsemble with a list of
batches) on a real MI355X.

Model m of K runs on instance m // (K // I): its own demand trace, initial state and cost / lead-time tables.  The bar is the
ensemble route's: BIT equality with single-model launches (`nic_small_rollout_fwd` / `_bwd_wgrad` / `_reduce`, `FusedRollout.run`) on
each model's weights and its instance's inputs, every stride - the instances' too - longer than its slice with NaN in the gaps; one
slot is also held to the reference's golden vectors."""
import copy
import functools

import pytest
import torch

from neural_inventory_control_amd import _lib, small_rollout as sr
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
from neural_inventory_control_amd.layout import EnvProblem, Table
from neural_inventory_control_amd.rollout import FusedRollout
from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
from test_gpu_small_ensemble import (DEV, NAN, PAD, ROW_PAD, _bits, _clones, _fresh_models, _golden_setting, _grads, _padded, _perturbed,
                                     _random_packed, _run_single, _same_grads, _Setting, _synthetic_data, _workload)

pytestmark = pytest.mark.gpu
TABLES = _lib.INSTANCE_TABLES
INST_PAD = dict(demand=8, state0=4, table=3)   # floats past an instance's slice of the stacked inputs
STATIC_KEYS = {"underage_costs": "cost", "holding_costs": "cost", "warehouse_holding_costs": "cost", "warehouse_edge_costs": "cost",
               "echelon_holding_costs": "cost", "lead_times": "lead", "warehouse_lead_times": "lead", "echelon_lead_times": "lead"}
COST_SCALE = (1.0, 2.25, 4.75)     # underage 4 -> 9 -> 19 on the one-store settings (one_store_lost.yml's grid)


# ---- launch level ------------------------------------------------------------------------------------------------------------------
def _instance_data(data, i, per_scenario):
    """instance i of a batch: its own demand and initial pipelines (seed 100 + i), costs scaled by COST_SCALE[i] (holding by 1 + i / 2),
    lead times i periods shorter (at least 1, at most the setting's: within the pipeline).  per_scenario: every table varies over the
    scenarios too."""
    gen = torch.Generator().manual_seed(100 + i)
    rand = lambda t: (0.5 + torch.rand(t.shape, generator=gen)).to(t.device)  # noqa: E731
    out = dict(data)
    for k in ("demands", "initial_inventories", "initial_warehouse_inventories", "initial_echelon_inventories"):
        if data.get(k) is not None:
            out[k] = data[k] * rand(data[k])
    for k, kind in STATIC_KEYS.items():
        v = data.get(k)
        if v is None:
            continue
        B = v.shape[0]
        b = torch.arange(B, device=v.device, dtype=torch.float32).view(B, *([1] * (v.dim() - 1)))
        if kind == "cost":
            v = v * (COST_SCALE[i] if k == "underage_costs" else 1.0 + 0.5 * i)
            out[k] = v * (1.0 + 0.01 * b) if per_scenario else v.clone()
        else:
            v = (v.float() - i).clamp_min(1.0)
            if per_scenario:   # every other scenario one period off, towards the inside of [1, the setting's lead time]
                v = v + torch.where(v >= 2.0, -1.0, 1.0) * (b % 2)
            out[k] = v.to(data[k].dtype)
    return out


def _instance_settings(chain, n_hidden, B, T, I, per_scenario):
    setting, data = _synthetic_data(chain, B, T)
    out = []
    for i in range(I):
        d = _instance_data(data, i, per_scenario)
        prob = EnvProblem(setting["problem_params"], d, DEV)
        if chain.startswith("one_store"):
            head, F, n_out = "softplus", prob.Ws, 1
        else:
            head, F, n_out = "serial", prob.Ws + prob.Ww + prob.E * prob.We, prob.E + 2
        dims = [F] + [32] * n_hidden + [n_out]
        assert sr.SmallRolloutPlan.supports(prob, head, dims)
        out.append(_Setting(prob, head, dims, d, T, 37.0, setting["problem_params"]["n_stores"]))
    for name in TABLES:   # the instances of a case have one layout, as the descriptor states it once
        t0 = getattr(out[0].prob, name)
        assert all((getattr(s.prob, name).tensor is None) == (t0.tensor is None) and getattr(s.prob, name).scn_stride == t0.scn_stride
                   for s in out), name
    assert out[0].prob.underage.scn_stride == (1 if per_scenario else 0)
    if I > 1:
        assert not torch.equal(out[0].prob.lead.tensor, out[1].prob.lead.tensor)   # (lead times differ within Ws)
        live = out[1].prob.lead.tensor[..., :B] if per_scenario else out[1].prob.lead.tensor   # (per-scenario: zero padding columns)
        assert float(live.max()) <= out[0].prob.Ws and float(live.min()) >= 1
    return out


def _stack(tensors, pad):
    """[I][numel + pad]: row i = tensors[i] flattened, NaN behind it"""
    n = tensors[0].numel()
    out = torch.full((len(tensors), n + pad), NAN, device=DEV)
    for i, t in enumerate(tensors):
        out[i, :n] = t.reshape(-1)
    return out


class _Instances:
    """the stacked inputs of I instances (what `share` names stays instance 0's, stride 0), the NicSmallInstances and the setting each
    instance's single-model launches run on"""

    def __init__(self, settings, share=()):
        self.I, s0 = len(settings), settings[0]
        self.keep, strides = {}, {}
        self.settings = []
        for s in settings:
            eff = copy.copy(s0)
            if "demand" not in share:
                eff.demand, eff.state0 = s.demand, s.state0
            if "tables" not in share:
                eff.prob = s.prob
            self.settings.append(eff)
        if "demand" not in share:
            self.keep["demand"] = _stack([s.demand for s in settings], INST_PAD["demand"])
            self.keep["state0"] = _stack([s.state0 for s in settings], INST_PAD["state0"])
            strides.update(demand=self.keep["demand"].stride(0), state0=self.keep["state0"].stride(0))
        if "tables" not in share:
            for name in TABLES:
                if getattr(s0.prob, name).tensor is not None:
                    self.keep[name] = _stack([getattr(s.prob, name).tensor for s in settings], INST_PAD["table"])
                    strides[name] = self.keep[name].stride(0)
        self.strides = strides
        self.inst = sr.instance_strides(self.I, **strides)

    def point(self, d):
        """the descriptor (built on instance 0's setting) <- the stacked inputs' addresses; strides and shapes stay"""
        for name, t in self.keep.items():
            if name in ("demand", "state0"):
                setattr(d, name, t.data_ptr())
            else:
                old = getattr(d, name)
                setattr(d, name, _lib.NicTable2(t.data_ptr(), old.loc_stride, old.scn_stride))
        return d

    def gaps_are_nan(self):
        pad = lambda name: INST_PAD[name] if name in INST_PAD else INST_PAD["table"]  # noqa: E731
        return all(bool(torch.isnan(t[:, t.shape[1] - pad(name):]).all()) and bool(torch.isfinite(t[:, :t.shape[1] - pad(name)]).all())
                   for name, t in self.keep.items())


def _run_instances(ins, packed, width, train=True, round_orders=False):
    """`_run_ensemble` of test_gpu_small_ensemble.py through the instances entry points"""
    s = ins.settings[0]
    K = packed.shape[0]
    w = _padded(K, s.P0, s.P0 + PAD["weights"])
    w[:, :s.P0] = packed
    d = ins.point(s.desc(w, width, round_orders))
    sl = sr.ensemble_slices(d)
    st = {k: sl[k] + PAD[k] for k in ("weights", "rewards", "final_state", "states", "hidden", "logits")}
    row = s.P0 + ROW_PAD
    st["slab"] = sl["slab_rows"] * row + PAD["slab"]
    st["grad"] = s.P0 + PAD["grad"]
    st["scratch"] = sr.small_rollout_reduce_scratch(sl["slab_rows"], s.P0, sl["rewards"]) + PAD["scratch"]
    ens = sr.ensemble_strides(K, **st)
    buf = dict(weights=w, rewards=_padded(K, sl["rewards"], st["rewards"], inside=0.0), final_state=_padded(K, 0, st["final_state"]),
               totals=torch.full((K, 2), NAN, device=DEV), scratch=_padded(K, 0, st["scratch"]))
    names = {}
    if train:
        for k in ("states", "hidden", "logits", "slab", "grad"):
            buf[k] = _padded(K, 0, st[k])
    hist = (buf["states"], buf["hidden"], buf["logits"]) if train else (None, None, None)
    sr.small_rollout_instances_fwd(d, ens, ins.inst, buf["rewards"], buf["final_state"], *hist)
    names["fwd"] = _lib.lib().nic_last_kernel().decode()
    n_el, ign = sl["rewards"], (s.T // 2) * s.prob.ldb
    if train:
        sr.small_rollout_instances_bwd_wgrad(d, ens, ins.inst, *hist, Table(s.g_reward, 0, 1), buf["slab"], row)
        names["bwd"] = _lib.lib().nic_last_kernel().decode()
        sr.small_rollout_ensemble_reduce(ens, buf["slab"], sl["slab_rows"], row, s.P0, buf["grad"], buf["rewards"], n_el, ign, buf["totals"],
                                         buf["scratch"])
    else:
        sr.small_rollout_ensemble_reduce(ens, None, 0, 0, 0, None, buf["rewards"], n_el, ign, buf["totals"], buf["scratch"])
    torch.cuda.synchronize()
    return buf, sl, st, row, names


def _compare_with_single_launches(ins, packed, width, train=True, round_orders=False):
    s = ins.settings[0]
    K, B, I = packed.shape[0], s.prob.B, ins.I
    R = K // I
    # the references first, and on them alone: the same weights on two instances give other totals, so a kernel that ignored an
    # offset could not pass what follows
    probe = sr.ensemble_slices(s.desc(packed[0].clone(), width, round_orders))
    row = s.P0 + ROW_PAD
    singles = [_run_single(ins.settings[m // R], packed[m], width, probe, row, train, round_orders) for m in range(K)]
    if I > 1:
        other = _run_single(ins.settings[1], packed[0], width, probe, row, train, round_orders)
        assert not torch.equal(other["totals"], singles[0]["totals"]) and not _bits(other["rewards"], singles[0]["rewards"])
    buf, sl, st, row, names = _run_instances(ins, packed, width, train, round_orders)
    assert sl == probe
    for tag, name in names.items():
        assert name.endswith(f"models={K},instances={I}>"), (tag, name)
    assert ("small_rollout16" in names["fwd"]) == (width == 16)
    size = dict(sl, slab=sl["slab_rows"] * row, grad=s.P0, scratch=0)
    keys = ("rewards", "final_state") + (("states", "hidden", "logits", "slab", "grad") if train else ())
    for m, one in enumerate(singles):
        for k in keys:
            assert _bits(buf[k][m, :size[k]], one[k]), (k, m)
        assert _bits(buf["totals"][m], one["totals"]), m
    # nothing wrote into a gap, nothing read one (the instances' gaps included): the live results are finite
    for k in keys + ("weights", "scratch"):
        assert bool(torch.isnan(buf[k][:, size[k] if k != "scratch" else st[k] - PAD[k]:]).all()), k
    assert ins.gaps_are_nan()
    T, ld, F = s.T, s.prob.ldb, s.plan.F
    assert bool(torch.isfinite(buf["rewards"][:, :sl["rewards"]].view(K, T, ld)[:, :, :B]).all())
    assert bool(torch.isfinite(buf["final_state"][:, :sl["final_state"]].view(K, F, ld)[:, :, :B]).all())
    assert bool(torch.isnan(buf["final_state"][:, :sl["final_state"]].view(K, F, ld)[:, :, B:]).all())
    assert bool(torch.isfinite(buf["totals"]).all())
    if train:
        assert bool(torch.isfinite(buf["grad"][:, :s.P0]).all())
        slab = buf["slab"][:, :size["slab"]].view(K, sl["slab_rows"], row)
        assert bool(torch.isfinite(slab[:, :, :s.P0]).all()) and bool(torch.isnan(slab[:, :, s.P0:]).all())
    return buf, sl, names


# (T, (I, R), what is shared, per-scenario tables, training): every (I, R) and both T; uniform and per-scenario tables; the demand
# per instance with every table shared and the reverse; an evaluation without histories and with rounded orders
RUNS = [(1, (1, 2), (), False, True), (7, (2, 1), ("tables",), False, True), (1, (2, 2), ("demand",), True, True),
        (7, (3, 2), (), True, True), (7, (2, 2), (), False, False)]


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("B", [16, 40, 100])
@pytest.mark.parametrize("n_hidden", [1, 2, 3])
@pytest.mark.parametrize("chain", ["one_store", "serial", "one_store_ws3", "serial_one_echelon"])
def test_instance_launches_equal_single_launches(chain, n_hidden, B, width):
    """the compiled-in chains and the run-time-structure ones at every depth, ragged last wavefronts at both widths"""
    for T, (I, R), share, per_scenario, train in RUNS:
        ins = _Instances(_instance_settings(chain, n_hidden, B, T, I, per_scenario), share)
        assert (ins.inst.demand == 0) == ("demand" in share) and (ins.inst.underage == 0) == ("tables" in share)
        _, _, names = _compare_with_single_launches(ins, _random_packed(ins.settings[0], I * R, 1000 * T + 10 * I + R), width, train=train,
                                                    round_orders=not train)
        shape = chain if chain in ("one_store", "serial") else "any"
        assert f"<{n_hidden},{shape}," in names["fwd"]


@pytest.mark.parametrize("width", [16, 32])
def test_one_slot_on_the_fixtures_own_data_meets_the_golden_vectors(width):
    """K = 2 models on I = 2 instances: instance 1 is the cfg1 fixture's own data and model 1 the fixture's parameters, instance 0
    carries other costs - slot 1 at the bars of tests/small_rollout_checks.py"""
    s, packed, g, idx = _golden_setting("cfg1_one_store_lost_vanilla")
    data = {k: v.to(DEV) for k, v in g.data.items()}
    dear = dict(data, underage_costs=data["underage_costs"] * 2.25, holding_costs=data["holding_costs"] * 1.5)
    c = g.fresh_config()
    other = _Setting(EnvProblem(c["problem_params"], dear, DEV), s.head, s.dims, dear, s.T, s.ub, s.n_stores)
    ins = _Instances([other, s])
    buf, sl, _ = _compare_with_single_launches(ins, _perturbed(packed, 2, 13, keep=1), width)
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


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
# what changes in an accepted request (K = 6 models on 3 instances, `nat`: the slices, `st`: the stacked inputs' strides) -> the reason
REFUSALS = {
    "no_instances": (lambda nat, st: dict(n=0), "n_instances must be at least 1"),
    "not_a_divisor": (lambda nat, st: dict(n=4), "n_instances must divide n_models"),
    # (more instances or replicas than a grid dimension takes need more models than an ensemble takes: its own limit is named first;
    # the validator's own wording is checked on the host, tests/test_small_instances_host.py)
    "too_many": (lambda nat, st: dict(n=65536, n_models=2 * 65536), "n_models must be 1..65535"),
    "negative_stride": (lambda nat, st: dict(holding=-1), "negative instance stride"),
    "short_demand": (lambda nat, st: dict(demand=nat["demand"] - 4), "demand stride shorter than (t0 + T) * ldb"),
    "short_state0": (lambda nat, st: dict(state0=nat["state0"] - 4), "state0 stride shorter than F * ldb"),
    "unaligned": (lambda nat, st: dict(demand=st["demand"] + 2), "multiples of 4 floats"),
    "null_table": (lambda nat, st: dict(wh_lead=5), "table whose pointer is NULL"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refused_requests_launch_nothing(what):
    """every refusal through the C ABI: non-zero, the limit named in nic_last_error, the outputs still NaN"""
    s, packed, _, _ = _golden_setting("cfg1_one_store_lost_vanilla")
    K, width = 6, 16
    w = _perturbed(packed, K, 14)
    ins = _Instances([s, s, s])
    d = ins.point(s.desc(w, width))
    sl = sr.ensemble_slices(d)
    row = sl["slab_row_stride"]
    make, reason = REFUSALS[what]
    change = make(dict(demand=s.T * s.prob.ldb, state0=s.plan.F * s.prob.ldb), ins.strides)
    n, n_models = change.pop("n", 3), change.pop("n_models", K)
    inst = sr.instance_strides(n, **{**ins.strides, **change})
    ens = sr.ensemble_strides(n_models, **{k: sl[k] for k in ("weights", "rewards", "final_state", "states", "hidden", "logits", "slab", "grad",
                                                             "scratch")})
    buf = {k: torch.full((K, sl[k]), NAN, device=DEV) for k in ("rewards", "final_state", "states", "hidden", "logits", "slab")}
    lib, stream = _lib.lib(), _lib.current_stream()
    hist = [buf[k].data_ptr() for k in ("states", "hidden", "logits")]
    calls = {"fwd": lambda: lib.nic_small_rollout_instances_fwd(d, ens, inst, buf["rewards"].data_ptr(), buf["final_state"].data_ptr(), *hist,
                                                                stream),
             "bwd_wgrad": lambda: lib.nic_small_rollout_instances_bwd_wgrad(d, ens, inst, *hist, Table(s.g_reward, 0, 1).t2(),
                                                                            buf["slab"].data_ptr(), row, stream)}
    for name, call in calls.items():
        assert call() != 0, name
        message = lib.nic_last_error().decode()
        assert message.startswith(f"nic_small_rollout_instances_{name}:") and reason in message, message
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool(torch.isnan(t).all()), k


def test_the_largest_ensemble_finds_its_instances():
    """65,535 models on 21,845 instances of 3 replicas, every instance with its own one-period demand: the kernels' multiply and shift
    at the largest model index (a wrong quotient shows only there), held to single-model launches on the models around the instance
    boundaries at both ends"""
    s = _instance_settings("one_store", 1, 16, 1, 1, False)[0]
    K, I, R, ld = 65535, 21845, 3, s.prob.ldb
    assert s.demand.numel() == ld
    factors = 1.0 + torch.arange(I, device=DEV, dtype=torch.float32).view(I, 1) / I
    demand = torch.full((I, ld + INST_PAD["demand"]), NAN, device=DEV)
    demand[:, :ld] = s.demand.view(1, ld) * factors
    packed = _random_packed(s, 1, 5).expand(K, -1).contiguous()
    d = s.desc(packed, 16)
    d.demand = demand.data_ptr()
    sl = sr.ensemble_slices(d)
    ens = sr.ensemble_strides(K, weights=sl["weights"], rewards=sl["rewards"], final_state=sl["final_state"])
    rewards, final = torch.zeros(K, sl["rewards"], device=DEV), torch.full((K, sl["final_state"]), NAN, device=DEV)
    sr.small_rollout_instances_fwd(d, ens, sr.instance_strides(I, demand=demand.stride(0)), rewards, final, None, None, None)
    assert _lib.lib().nic_last_kernel().decode().endswith("models=65535,instances=21845>")
    torch.cuda.synchronize()
    for m in (0, 2, 3, 5, 6, 32766, 32767, 32768, 65531, 65532, 65534):
        one = copy.copy(s)
        one.demand = demand[m // R, :ld].clone().view(1, 1, ld)
        want = _run_single(one, packed[m], 16, sl, sl["slab_row_stride"], train=False)
        assert _bits(rewards[m], want["rewards"]) and _bits(final[m], want["final_state"]), m
    assert not _bits(rewards[K - 1], rewards[K - 4]) and _bits(rewards[K - 1], rewards[K - 3])   # (the last instance's three replicas)


# ---- engine level ------------------------------------------------------------------------------------------------------------------
IGN = 2


@functools.lru_cache(maxsize=None)
def _engine_instances(workload, I, B, T, n_batches=1):
    """n_batches lists of I batch dicts: slices of one pool (other demand seeds), underage and holding costs scaled per instance"""
    setting, policy, obs, _, pool = _workload(workload, n_batches * I * B, T)
    out = []
    for j in range(n_batches):
        row = []
        for i in range(I):
            lo = (j * I + i) * B
            data = {k: v[lo:lo + B] for k, v in pool.items()}
            data["underage_costs"] = data["underage_costs"] * COST_SCALE[i]
            data["holding_costs"] = data["holding_costs"] * (1.0 + 0.5 * i)
            row.append(data)
        out.append(row)
    assert not torch.equal(out[0][0]["demands"], out[0][1]["demands"])
    return setting, obs, out


@pytest.mark.parametrize("workload,I,R", [("cfg1", 2, 2), ("cfg4", 3, 1)])
def test_engine_equals_single_model_engines_on_each_models_instance(workload, I, R):
    B, T, K = 96, 8, I * R
    setting, obs, batches = _engine_instances(workload, I, B, T, 2)
    models = _fresh_models(workload, 2 * I * B, T, tuple(range(1, K + 1)))
    alone = _clones(models)
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    singles = [FusedRollout(m, setting["problem_params"], DEV) for m in alone]
    for datas, train in ((batches[0], True), (batches[0], False), (batches[1], True), (tuple(batches[1]), False)):
        tot, rep = ens.run(datas, T, IGN, train=train, observation_params=obs)
        assert tuple(tot.shape) == tuple(rep.shape) == (K,)
        for m, eng in enumerate(singles):
            t1, r1 = eng.run(datas[m // R], T, IGN, train=train, observation_params=obs)
            assert torch.equal(tot[m], t1) and torch.equal(rep[m], r1), (m, float(tot[m]), float(t1))
            assert torch.equal(ens.rewards[m], eng.rewards)
        if train:
            assert _same_grads(_grads(models), _grads(alone))
        assert all(ens.last_kernels[k].endswith(f"models={K},instances={I}>") for k in ("fwd",) + (("bwd",) if train else ()))
    assert not torch.equal(tot[0], tot[K - 1])
    # a caller's stacked trace of exactly the engine's shape is read in place
    stacked = ens.inst_demand.clone()
    tot2, _ = ens.run(batches[1], T, IGN, train=False, observation_params=obs, demand_soa=stacked)
    assert torch.equal(tot2, tot)
    with pytest.raises(ValueError, match=r"demand_soa of a list of instances must be \[I\]\[T_total\]\[1\]\[ldb\]"):
        ens.run(batches[1], T, IGN, train=False, observation_params=obs, demand_soa=stacked[0])
    # the one-batch path through the same engine is what it was
    tot3, _ = ens.run(batches[0][0], T, IGN, train=False, observation_params=obs)
    for m, eng in enumerate(singles):
        assert torch.equal(tot3[m], eng.run(batches[0][0], T, IGN, train=False, observation_params=obs)[0])
    assert ens.last_kernels["fwd"].endswith(f"models={K}>")


def _adam(ens, lrs):
    P = sum(p.numel() for p in ens.models[0].parameters())
    return EnsembleAdam(ens.n_models, P, DEV, lr=list(lrs), param_shapes=ens.param_shapes)


@pytest.mark.parametrize("use_graph", [False, True])
def test_three_train_steps_equal_per_instance_ensembles(use_graph):
    """K = 4 models on I = 2 instances with one EnsembleAdam against two 2-model ensembles, one per instance, each with its own"""
    I, R, B, T = 2, 2, 96, 8
    K = I * R
    setting, obs, batches = _engine_instances("cfg1", I, B, T, 3)
    lrs = (1e-2, 3e-3, 1e-3, 3e-2)
    models = _fresh_models("cfg1", 3 * I * B, T, (31, 32, 33, 34))
    alone = _clones(models)
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    ens.use_graph = use_graph
    ens.bind_parameters()
    opt = _adam(ens, lrs)
    got = [torch.stack(ens.train_step(datas, T, IGN, opt, obs)) for datas in batches]
    torch.cuda.synchronize()
    if use_graph:
        assert len(ens._graphs) == 1 and ens._replay.demand is None and ens._replay.prob is None   # (nothing staged, nothing pinned)
    for i in range(I):
        part = SmallPolicyEnsemble(alone[i * R:(i + 1) * R], setting["problem_params"], DEV)
        part.bind_parameters()
        popt = _adam(part, lrs[i * R:(i + 1) * R])
        for step, datas in enumerate(batches):
            want = torch.stack(part.train_step(datas[i], T, IGN, popt, obs))
            assert torch.equal(got[step][:, i * R:(i + 1) * R], want), (step, i)
        torch.cuda.synchronize()
        assert _bits(ens.weights[i * R:(i + 1) * R], part.weights)
        assert _bits(opt.exp_avg[i * R:(i + 1) * R], popt.exp_avg) and _bits(opt.exp_avg_sq[i * R:(i + 1) * R], popt.exp_avg_sq)
    assert not torch.equal(ens.weights[0], ens.weights[R])


@pytest.mark.parametrize("use_graph", [False, True])
def test_one_batch_and_instance_steps_interleaved_equal_a_fresh_engine_per_step(use_graph):
    """One engine takes a dict, a list, a dict, a list (evaluation, the batches of the step before it, then new ones) through its
    one step path; its twin is a fresh eager engine for EVERY step on the twin's models and the twin's EnsembleAdam, so nothing of
    one step - initial state, pinned problem, stacked tables, captures - can reach the next.  40 scenarios leave padded lanes."""
    I, R, B, T = 2, 2, 40, 8
    K = I * R
    setting, obs, lists = _engine_instances("cfg1", I, B, T, 4)
    steps = [(lists[0][1], True), (lists[1], True), (lists[2][0], True), (lists[1], False), (lists[3], True)]
    lrs = (1e-2, 3e-3, 1e-3, 3e-2)
    models = _fresh_models("cfg1", 4 * I * B, T, (61, 62, 63, 64))
    alone = _clones(models)
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    ens.use_graph = use_graph
    ens.bind_parameters()
    opt, topt = _adam(ens, lrs), None
    for step, (data, train) in enumerate(steps):
        twin = SmallPolicyEnsemble(alone, setting["problem_params"], DEV)
        twin.bind_parameters()   # (the values the step before left in the twin's models)
        topt = _adam(twin, lrs) if topt is None else topt
        if train:
            got, want = ens.train_step(data, T, IGN, opt, obs), twin.train_step(data, T, IGN, topt, obs)
        else:
            got, want = (e.run(data, T, IGN, train=False, observation_params=obs) for e in (ens, twin))
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), step
        assert torch.equal(ens.weights, twin.weights), step
        assert ("instances" in ens.last_kernels["fwd"]) == isinstance(data, list), (step, ens.last_kernels)
        assert ens.last_kernels["fwd"] == twin.last_kernels["fwd"]
    assert torch.equal(opt.exp_avg, topt.exp_avg) and torch.equal(opt.exp_avg_sq, topt.exp_avg_sq)
    assert opt.steps().tolist() == [4] * K and not torch.equal(ens.weights[0], ens.weights[R])
    if use_graph:   # (the dict shape's second step and both of the list shape's later ones were replayed)
        assert len(ens._shapes) == 1 and sum(len(st.replay.graphs) for st in [ens._shape, *ens._shapes.values()]) == 3


def test_fit_over_lists_of_instances_returns_histories_per_model():
    I, R, B, T = 2, 2, 64, 6
    K = I * R
    setting, obs, batches = _engine_instances("cfg1", I, B, T, 3)
    ens = SmallPolicyEnsemble(_fresh_models("cfg1", 3 * I * B, T, (41, 42, 43, 44)), setting["problem_params"], DEV)
    ens.bind_parameters()
    train_hist, dev_hist = ens.fit(batches[:2], batches[2:], 2, T, T, IGN, _adam(ens, (1e-2,) * K), obs)
    assert tuple(train_hist.shape) == tuple(dev_hist.shape) == (2, K)
    assert bool(torch.isfinite(train_hist).all()) and bool(torch.isfinite(dev_hist).all())
    # the sample count is per instance: the dev history is the reported cost per (scenario, reported period, store) of one batch
    _, rep = ens.run(batches[2], T, IGN, train=False, observation_params=obs)
    assert torch.allclose(dev_hist[1], rep / float(B * (T - IGN) * setting["problem_params"]["n_stores"]), rtol=1e-6)
    assert tuple(ens.best_dev.shape) == (K,)


def test_engine_refuses_mismatched_instances():
    B, T = 64, 6
    setting, obs, batches = _engine_instances("cfg1", 2, B, T, 1)
    datas = batches[0]
    models = _fresh_models("cfg1", 2 * B, T, (51, 52, 53))
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    with pytest.raises(ValueError, match="2 problem instances do not divide 3 models"):
        ens.run(datas, T, IGN, train=False, observation_params=obs)
    ens = SmallPolicyEnsemble(models[:2], setting["problem_params"], DEV)
    short = {k: v[:B - 8] for k, v in datas[1].items()}
    with pytest.raises(ValueError, match="instance 1: 56 scenarios, instance 0 has 64"):
        ens.run([datas[0], short], T, IGN, train=False, observation_params=obs)
    clipped = dict(datas[1], demands=datas[1]["demands"][:, :, :T - 1].contiguous())
    with pytest.raises(ValueError, match="instance 1: a demand trace of 5 periods"):
        ens.run([datas[0], clipped], T - 1, IGN, train=False, observation_params=obs)
    varied = dict(datas[1], underage_costs=datas[1]["underage_costs"] * torch.linspace(1, 2, B, device=DEV)[:, None])
    with pytest.raises(ValueError, match="instance 1: table 'underage' is per-scenario, instance 0's is uniform"):
        ens.run([datas[0], varied], T, IGN, train=False, observation_params=obs)
