"""End-to-end parity on a real MI355X, all through the C ABI:

  * `FusedRollout` (whole-horizon HIP forward + analytic backward) against the golden vectors of the reference for
    every MLP configuration: per-period reward, per-scenario total cost (<= 1e-5 relative, north_star), final state,
    and d(mean_loss)/d(theta) per parameter tensor;
  * the general route (`Simulator.step` as an autograd-aware HIP kernel + HipLinear policies) for ALL configurations,
    including the closed-form policies;
  * the reference's shipped checkpoint known answer (6.854347) through the HIP path;
  * size-independent properties at BASELINE's full sizes (batch-size independence, stock conservation).
"""
import numpy as np
import pytest
import torch

import grad_parity_log

from golden_io import Golden, ZERO_LEAD_CASES, case_names, check_slim_inputs, slim_case_names
from neural_inventory_control_amd import _lib
from neural_inventory_control_amd.data_handling import DatasetCreator, DeviceBatches, MyDataset, Scenario
from neural_inventory_control_amd.environment import Simulator
from neural_inventory_control_amd.loss_functions import PolicyLoss
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.policy_layers import materialize_linears
from neural_inventory_control_amd.rollout import FusedRollout
from neural_inventory_control_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# state after T periods of a random-init policy in the loop: f32 round-off of the policy GEMMs (different summation order
# than the CPU reference) is amplified by the recurrence; costs stay within 1e-5, individual pipeline slots within 1e-4
STATE_TOL = dict(rtol=1e-4, atol=2e-3)
MLP_CASES = [n for n in case_names() if n.endswith("vanilla")]
# Gradient bar: d(mean_loss)/d(theta) per parameter tensor within 1e-5 relative L2 (north_star) of the reference's golden gradient for EVERY
# configuration (measured on MI355X: <= 1.3e-6 on all fixtures, the 3-warehouse x 64-store one included).  Nothing is
# widened per case; where the two sides sum 10^5 fp32 terms per weight in different orders (benchmark width and horizon)
# the criterion is the fp64 referee below instead of a wider band.
GRAD_TOL = 1e-5


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / (b.double().norm() + 1e-30))


def _model(g, c, scenario=None):
    class _Sc:  # the factory only reads problem_params / store_params of the scenario
        pass
    sc = scenario or _Sc()
    if scenario is None:
        sc.problem_params = c["problem_params"]
        sc.store_params = {"demand": {"mean": [float(x) for x in np.atleast_1d(g.z["mutated_mean"])]}}
    if g.forecaster is not None:
        # quantile policies load their frozen forecaster from nn_params['forecaster_location'] (a file of the reference's
        # tree); the fixture carries its weights, written to a temporary file in the reference's own format
        import os
        import tempfile
        path = os.path.join(tempfile.mkdtemp(), "forecaster.pt")
        torch.save(g.forecaster, path)
        c["nn_params"]["forecaster_location"] = path
    model = NeuralNetworkCreator().create_neural_network(sc, c["nn_params"], device=DEV)
    model.warehouse_upper_bound = g.tensor("warehouse_upper_bound").to(DEV)
    return model


def _load(model, g):
    if g.params:  # (just_in_time never materialises its unused net: nothing to load)
        model.load_state_dict({k: v.to(DEV) for k, v in g.params.items()})


def _sorted_grad_keys(ref):
    return sorted(ref.keys(), key=lambda s: (int(s.split(".")[2]), s.split(".")[3] != "weight"))


class _Expected:
    """rewards [T][B], total, reported, final state, gradients by parameter name: the golden numbers, or (ZERO_LEAD_CASES) the
    oracle's with zero-lead orders dropped."""

    def __init__(self, g, c):
        from oracle import inventory_oracle as orc
        if g.name not in ZERO_LEAD_CASES:
            self.rewards, self.total, self.reported = g.tensor("rewards"), float(g.z["total"]), float(g.z["reported"])
            self.final, self.grads = g.states(c["periods"]), g.grads
            return
        pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"))
        res, _, grads = orc.train_step_gradients(pol, c["periods"], c["problem_params"], g.data, c["observation_params"],
                                                 c["ignore"], zero_lead_orders="drop")
        assert abs(float(res.total) - float(g.z["total"])) > 1e-3 * abs(float(g.z["total"]))   # the modes do differ here
        self.rewards, self.total, self.reported = res.per_period, float(res.total), float(res.reported)
        self.final = {k: v.detach() for k, v in res.final_obs.items() if k.endswith("inventories")}
        names = [f"net.{m}.{2 * i}.{w}" for m in orc.GNN_MODULES for i in range(3) for w in ("weight", "bias")]
        assert sorted(names) == sorted(g.grads)
        self.grads = dict(zip(names, grads))


def _check_grads(model, g, tol, ref=None):
    ref = g.grads if ref is None else ref
    named = dict(model.named_parameters())
    worst = 0.0
    for k in _sorted_grad_keys(ref):
        got = named[k].grad
        assert got is not None, k
        rel = float((got.cpu() - ref[k]).norm() / (ref[k].norm() + 1e-30))
        worst = max(worst, rel)
        assert rel <= tol, (k, rel)
    grad_parity_log.note(worst, tol)
    return worst


@pytest.mark.parametrize("name", MLP_CASES)
def test_fused_rollout_matches_reference(name):
    g = Golden(name)
    c = g.fresh_config()
    model = _model(g, c)
    eng = FusedRollout(model, c["problem_params"], DEV)
    data = {k: v.to(DEV) for k, v in g.data.items()}
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if c["policy"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)
    eng.materialize(F)
    _load(model, g)
    total, reported = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
    torch.cuda.synchronize()
    rewards = eng.per_period_rewards().cpu()
    ref_r = g.tensor("rewards")
    torch.testing.assert_close(rewards, ref_r, rtol=1e-5, atol=1e-4)
    # north_star: per-scenario total cost within 1e-5 relative
    tot_b, ref_b = rewards.double().sum(dim=0), ref_r.double().sum(dim=0)
    assert float(((tot_b - ref_b).abs() / ref_b.abs().clamp_min(1e-9)).max()) <= 1e-5
    assert abs(float(total) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))
    assert abs(float(reported) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
    final = eng.final_state()
    for k, v in g.states(c["periods"]).items():
        torch.testing.assert_close(final[k].cpu(), v, **STATE_TOL)
    _check_grads(model, g, GRAD_TOL)
    # evaluation mode (no activations kept) gives the same costs
    t2, r2 = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
    assert float(t2) == float(total) and float(r2) == float(reported)


DATA_DRIVEN_CASES = [n for n in case_names() if n.endswith("data_driven")]


@pytest.mark.parametrize("route", ["horizon", "periods"])
@pytest.mark.parametrize("name", DATA_DRIVEN_CASES)
def test_data_driven_engine_matches_reference(name, route):
    """SURVEY 8 f4 on the MLP engine (round 3): `FusedRollout` with the data_driven head - the past-demand window, costs,
    days-from-christmas and lead-time rows appended to every period's state block, ReLU + adjacency mask + proportional
    allocation of the warehouses' pipelines in one head kernel (`nic_head_data_driven_fwd/bwd`), profit objective, demand
    trace entered at period_shift - against the reference-generated real-data fixtures: rewards, totals, final state,
    gradients at the usual bars; evaluation mode and the Trainer's own routing agree.  Both routes: `horizon` = all periods in
    one launch per direction (round 4, csrc/horizon_rollout.hip: what small batches take by default), `periods` = the
    per-period kernels."""
    assert DATA_DRIVEN_CASES
    g = Golden(name)
    c = g.fresh_config()
    model = _model(g, c)
    assert FusedRollout.supports(model) and FusedRollout.observation_ok(model, c["observation_params"], g.data)
    eng = FusedRollout(model, c["problem_params"], DEV)
    eng.use_horizon = route == "horizon"
    assert eng.head == "data_driven"
    data = {k: v.to(DEV) for k, v in g.data.items()}
    eng.materialize(g.params["net.master.0.weight"].shape[1])
    _load(model, g)
    total, reported = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
    torch.cuda.synchronize()
    assert eng.small is None and eng.dims[0] == g.params["net.master.0.weight"].shape[1]
    assert (eng.horizon is not None) == (route == "horizon")
    block = (lambda t: eng.hz_X[:, t]) if route == "horizon" else (lambda t: eng.states[t])   # one period's input rows
    rewards = eng.per_period_rewards().cpu()
    ref_r = g.tensor("rewards").float()
    torch.testing.assert_close(rewards, ref_r, rtol=1e-5, atol=2e-2)
    assert abs(float(total) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))
    assert abs(float(reported) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
    final = eng.final_state()
    for k, v in g.states(c["periods"]).items():
        torch.testing.assert_close(final[k].cpu(), v.float(), rtol=2e-6, atol=2e-3)
    # every period's observation block is the reference's flattened feature vector (inventories | window | costs | ...)
    for t in (0, c["periods"] // 2, c["periods"] - 1):
        feats = g.features(t)
        o = eng.F_dyn
        S, P_ = c["problem_params"]["n_stores"], c["observation_params"]["demand"]["past_periods"]
        got = block(t)[o:o + S * P_, :c["n"]].t().reshape(c["n"], S, P_).cpu()
        assert torch.equal(got, feats["past_demands"]), t
        o += S * P_ + 2 * S
        D = feats["days_from_christmas"].shape[1]
        assert torch.equal(block(t)[o:o + D, :c["n"]].t().cpu(), feats["days_from_christmas"]), t
        if route == "horizon":   # the state rows the kernel left for the backward are the reference's inventories before period t
            for k, v in g.states(t).items():
                rows = block(t)[:eng.F_store] if k == "store_inventories" else block(t)[eng.F_store:eng.F_dyn]
                torch.testing.assert_close(rows[:, :c["n"]].t().reshape(v.shape).cpu(), v.float(), rtol=2e-6, atol=2e-3)
    worst = _check_grads(model, g, GRAD_TOL)
    print(f"{name}: worst relative gradient error {worst:.2e}")
    t2, r2 = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
    assert float(t2) == float(total) and float(r2) == float(reported)
    # the Trainer picks this engine by itself for the real-data observation (and keeps the generic loop for other policies)
    tr = Trainer(device=DEV)
    model.zero_grad()
    tot3, _ = tr.simulate_batch(PolicyLoss(), Simulator(device=DEV), model, c["periods"], c["problem_params"], data,
                                c["observation_params"], c["ignore"], False)
    assert any(isinstance(e, FusedRollout) for e in tr._engines.values())
    (tot3 / (c["n"] * c["periods"] * c["problem_params"]["n_stores"])).backward()
    _check_grads(model, g, GRAD_TOL)


def test_data_driven_engine_graph_replay_and_discrete_evaluation():
    """The data_driven engine's launch sequence replayed from HIP graphs (the observation rows are written outside the
    captured region): same totals and gradients as eager launches, also after the batch contents change; and evaluation with
    discrete allocation (orders rounded half to even between head and env step, trainer.py:201-202) against the oracle."""
    from oracle import inventory_oracle as orc
    g = Golden("f4_real_many_warehouses_data_driven")
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    data2 = dict(data)
    data2["demands"] = (data["demands"] * 1.2 + 0.5).contiguous()
    out = {}
    for mode in ("eager", "graph"):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.use_horizon = False   # (the per-period launch sequence is what gets captured; the whole-horizon route is two launches)
        eng.use_graph = mode == "graph"
        eng.materialize(eng.input_rows(data, c["observation_params"]))
        _load(model, g)
        res = []
        for d in (data, data2, data):
            total, rep = eng.run(d, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
            torch.cuda.synchronize()
            res.append((float(total), float(rep), [p.grad.clone() for p in model.parameters()]))
        out[mode] = res
        if mode == "graph":
            assert len(eng._graphs) == 2
    for a, b in zip(out["eager"], out["graph"]):
        assert a[0] == b[0] and a[1] == b[1]
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x, y)
    assert out["eager"][0][0] != out["eager"][1][0] and out["eager"][0][0] == out["eager"][2][0]
    with torch.no_grad():
        total, reported = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"],
                                  discrete_allocation=True)
    pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"))
    with torch.no_grad():
        ref = orc.rollout(pol, c["periods"], c["problem_params"], g.data, c["observation_params"], c["ignore"],
                          discrete_allocation=True)
    assert abs(float(total) - float(ref.total)) <= 1e-5 * abs(float(ref.total))
    assert abs(float(reported) - float(ref.reported)) <= 1e-5 * abs(float(ref.reported))
    assert float(total) != out["eager"][0][0]
    # the whole-horizon route: same training results as the per-period launches up to the layers' summation order, also when the
    # batch contents change between runs of one engine; and its own discrete-allocation evaluation
    model = _model(g, c)
    hz_eng = FusedRollout(model, c["problem_params"], DEV)
    hz_eng.materialize(hz_eng.input_rows(data, c["observation_params"]))
    _load(model, g)
    for d, want in zip((data, data2, data), out["eager"]):
        tot, rep = hz_eng.run(d, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
        assert hz_eng.horizon is not None
        assert abs(float(tot) - want[0]) <= 2e-6 * abs(want[0]) and abs(float(rep) - want[1]) <= 2e-6 * abs(want[1])
        for p_, y in zip(model.parameters(), want[2]):
            assert float((p_.grad - y).abs().max()) <= 1e-5 * float(y.abs().max()) + 1e-9
    with torch.no_grad():
        tot, rep = hz_eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"],
                              discrete_allocation=True)
    assert abs(float(tot) - float(ref.total)) <= 1e-5 * abs(float(ref.total))
    assert abs(float(rep) - float(ref.reported)) <= 1e-5 * abs(float(ref.reported))


def test_data_driven_epochs_engine_follows_generic_route():
    """Two training epochs + an evaluation pass of the real-data setting's shape (synthetic stand-in files, 21 stores x 3
    warehouses, past-demand window of 16, datasets split by period) through `Trainer.do_one_epoch` with ragged batches (16, 16, 8
    products): the MLP engine with the data_driven head against the generic route (Simulator.step + autograd), step for step."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    setting, policy, _, _, _ = workloads.get("real_data_driven")
    n, T = 40, 12
    obs = defaultdict(lambda: None, setting["observation_params"])
    shift = obs["demand"]["period_shift"]
    sc = Scenario(shift + T, setting["problem_params"], setting["store_params"], setting["warehouse_params"],
                  setting["echelon_params"], n, obs, setting["seeds"], device=DEV)
    (ds,) = DatasetCreator().create_datasets(sc, split=True, by_period=True, periods_for_split=[f"(0, {shift + T})"])
    runs = {}
    for fused in (True, False):
        torch.manual_seed(5)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        tr, sim = Trainer(device=DEV), Simulator(device=DEV)
        tr.use_fused_rollout = fused
        loader = DeviceBatches(ds, 16, shuffle=False, device=DEV)
        batch = next(iter(loader))
        o, _ = sim.reset(T, setting["problem_params"], batch, obs)
        with torch.no_grad():
            o = dict(o)
            o["internal_data"] = sim._internal_data
            model(o)                                    # materialises the lazy first layer identically on both routes
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = [tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, T, setting["problem_params"], obs, train=True,
                                  ignore_periods=3) for _ in range(2)]
        ev = tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, T, setting["problem_params"], obs, train=False,
                             ignore_periods=3)
        assert any(isinstance(e, FusedRollout) for e in tr._engines.values()) == fused
        runs[fused] = (losses, ev, [p.detach().clone() for p in model.parameters()])
    for a, b in zip(runs[True][0] + [runs[True][1]], runs[False][0] + [runs[False][1]]):
        assert abs(a[0] - b[0]) <= 1e-5 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-5 * abs(b[1]), (a, b)
    # parameters after six Adam steps: Adam divides every gradient element by its own running magnitude, so an element whose
    # gradient is rounding noise (|g| ~ 1e-9) moves by a full step in a direction the two routes' summation orders decide -
    # nearly all elements agree to 2e-6, a handful (<= 0.01 %) may differ by a few percent of ONE step (lr = 1e-3)
    for x, y in zip(runs[True][2], runs[False][2]):
        bad = (x - y).abs() > 2e-6 + 1e-4 * y.abs()
        assert int(bad.sum()) <= max(1, x.numel() // 10000), (int(bad.sum()), x.numel())
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-4)
    assert runs[True][0][0][0] != runs[True][0][1][0]      # the optimizer moved the policy between the epochs


@pytest.mark.parametrize("name", MLP_CASES)
def test_hybrid_host_sweep_on_device(name):
    """tests/host_rollout.py on the device: the HIP env-step and head kernels (through the C ABI) composed in the engine's
    sweep order with torch matmuls instead of the MFMA GEMMs — isolates the adjoint of the kernel composition from GEMM
    summation order.  Same bars as the CPU run of the harness (tests/test_host_rollout.py)."""
    import kernel_checks as kc
    from test_host_rollout import run_case
    g, c, out, worst = run_case(kc.HipBackend(), name)
    assert abs(float(out["total"]) - float(g.z["total"])) <= 1e-6 * abs(float(g.z["total"]))
    torch.testing.assert_close(out["rewards"].cpu(), g.tensor("rewards"), rtol=2e-6, atol=1e-5)
    assert worst <= 5e-6, worst


QUANTILE_TRAINABLE = ["f4_real_one_store_fixed_quantile", "f4_real_one_store_transformed_nv"]


def _order_up_to_knife_edges(g, c):
    """Scenarios of a quantile-policy fixture that sit on a clamp knife edge at some period.  An order-up-to policy facing a
    zero-demand week with unchanged features wants `level - position` = 0 up to rounding (the position IS last period's level),
    and `clip(., min=0)` passes the gradient iff that noise is >= 0: the reference's own outcome there depends on float64
    rounding of its state, no other arithmetic can reproduce it.  Found with the oracle in float64; structural exact zeros and
    clearly negative / positive gaps are not knife edges."""
    from oracle import inventory_oracle as orc
    pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"),
                                     dtype=torch.float64, forecaster_state=g.forecaster)
    probe = []
    with torch.no_grad():
        orc.rollout(pol, c["periods"], c["problem_params"], {k: v.double() for k, v in g.data.items()},
                    c["observation_params"], c["ignore"], probe=probe)
    bad = torch.zeros(c["n"], dtype=torch.bool)
    for level, gap in probe:
        bad |= ((gap.abs() <= 1e-4 * (level.abs() + 1.0))).any(dim=1)
    return bad


@pytest.mark.parametrize("route", ["tape", "generic"])
@pytest.mark.parametrize("name", QUANTILE_TRAINABLE)
def test_quantile_policy_gradients_with_knife_edge_exclusion_and_fp64_referee(name, route):
    """Gradient parity of the trainable quantile policies through the HIP simulator - on the generic route (Simulator.step +
    autograd, period by period) and on the tape route the Trainer picks by itself (round 4: all levels in one batched pass, one
    whole-horizon launch per direction, tape_rollout.py).  Two effects make a plain band
    meaningless here and each gets its own mechanism: (1) knife-edge scenarios (see _order_up_to_knife_edges) are excluded,
    counted and bounded; (2) the base-stock level is an interpolation between ADJACENT outputs of the frozen float32
    forecaster, so d level / d quantile carries the forecaster's rounding amplified by cancellation.  The criterion is an fp64
    referee with a measured noise floor: the reference's float32 arithmetic is re-run with the forecaster's weights perturbed by
    one ulp (8 draws); its largest distance from the float64 evaluation is what float32 rounding of the forecaster can do to
    this gradient (2e-6 .. 2e-5 on the fixed-quantile fixture), and the HIP path must stay within twice that (or inside the
    2e-5 bar)."""
    from oracle import inventory_oracle as orc
    g = Golden(name)
    c = g.fresh_config()
    bad = _order_up_to_knife_edges(g, c)
    ok = ~bad
    assert int(ok.sum()) >= c["n"] // 2, f"{int(bad.sum())} of {c['n']} scenarios on a knife edge"
    sub = {k: v[ok].contiguous() for k, v in g.data.items()}
    n_ok = int(ok.sum())
    norm = n_ok * c["periods"] * c["problem_params"]["n_stores"]
    # the reference's arithmetic (oracle, float32 with its float64 interpolation) and the float64 referee on the same subset
    pol32 = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"),
                                       forecaster_state=g.forecaster)
    res32, _, g32 = orc.train_step_gradients(pol32, c["periods"], c["problem_params"], sub, c["observation_params"], c["ignore"])
    perturbed = []
    for trial in range(1, 8):
        gen = torch.Generator().manual_seed(trial)
        fs = {k: (v * (1 + 6e-8 * torch.randn(v.shape, generator=gen))).float() for k, v in g.forecaster.items()}
        pp = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"),
                                        forecaster_state=fs)
        perturbed.append(orc.train_step_gradients(pp, c["periods"], c["problem_params"], sub, c["observation_params"],
                                                  c["ignore"])[2])
    pol64 = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"),
                                       dtype=torch.float64, forecaster_state=g.forecaster)
    _, _, g64 = orc.train_step_gradients(pol64, c["periods"], c["problem_params"], {k: v.double() for k, v in sub.items()},
                                         c["observation_params"], c["ignore"])
    model = _model(g, c)
    data = {k: v.to(DEV) for k, v in sub.items()}
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    tr.use_fused_rollout = route == "tape"
    obs, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
    with torch.no_grad():
        o = dict(obs)
        o["internal_data"] = sim._internal_data
        model(o)
    _load(model, g)
    model.zero_grad()
    total, _ = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data, c["observation_params"],
                                 c["ignore"], False)
    assert (type(getattr(tr, "_last_engine", None)).__name__ == "TapeRollout") == (route == "tape")
    (total / norm).backward()
    torch.cuda.synchronize()
    assert abs(float(total) - float(res32.total)) <= 1e-5 * abs(float(res32.total))
    named = dict(model.named_parameters())
    for i, (k, r32, r64) in enumerate(zip(_sorted_grad_keys(g.grads), g32, g64)):
        if float(r64.abs().max()) == 0.0:
            assert float(named[k].grad.abs().max()) == 0.0, k
            continue
        e_hip = _rel(named[k].grad, r64)
        e_ref = max([_rel(r32, r64)] + [_rel(p[i], r64) for p in perturbed])
        print(f"{k}: |HIP - fp64| = {e_hip:.2e}  float32 noise floor of the reference (1-ulp forecaster perturbations) = "
              f"{e_ref:.2e}  ({n_ok} of {c['n']} scenarios)")
        assert e_hip <= max(2.0 * e_ref, GRAD_TOL), (k, e_hip, e_ref)


@pytest.mark.parametrize("name", case_names())
def test_simulator_autograd_route_matches_reference(name):
    """reference-style loop: model(observation) -> simulator.step(action) -> loss -> backward (trainer.py:190-216)."""
    g = Golden(name)
    c = g.fresh_config()
    model = _model(g, c)
    data = {k: v.to(DEV) for k, v in g.data.items()}
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    tr.use_fused_rollout = False
    obs, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
    with torch.no_grad():
        o = dict(obs)
        o["internal_data"] = sim._internal_data
        model(o)  # materialises the lazy layers
    _load(model, g)
    model.zero_grad()
    total, reported = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data,
                                        c["observation_params"], c["ignore"], False)
    if total.requires_grad:  # (quantile_nv / returns_nv / just_in_time have nothing to train)
        (total / (c["n"] * c["periods"] * c["problem_params"]["n_stores"])).backward()
    torch.cuda.synchronize()
    want = _Expected(g, c)
    assert abs(float(total) - want.total) <= 1e-5 * abs(want.total)
    assert abs(float(reported) - want.reported) <= 1e-5 * abs(want.reported)
    for k, v in want.final.items():
        torch.testing.assert_close(sim.observation[k].cpu(), v.float(), **STATE_TOL)
    assert int(sim.observation["current_period"]) == c["periods"]
    if name not in QUANTILE_TRAINABLE:  # (those: test_quantile_policy_gradients_with_knife_edge_exclusion_and_fp64_referee)
        _check_grads(model, g, GRAD_TOL, want.grads)


TAPE_CASES = [n for n in case_names() if n.startswith("f4_real") and not n.endswith("data_driven")]


@pytest.mark.parametrize("name", TAPE_CASES)
def test_tape_engine_matches_reference(name):
    """SURVEY 8 f4, the policies that need no network inside the period loop (round 4, tape_rollout.py): the four quantile policies
    (all levels from ONE batched pass of the frozen forecaster, order-up-to + env step in one launch of the whole-horizon kernel)
    and just-in-time on one store and on 21 stores x 3 warehouses (all orders from one batched gather of future demand, one launch)
    - through `Trainer.simulate_batch`, which picks the engine by itself - against the reference-generated fixtures: per-period
    rewards, totals, final state; gradients of the trainable ones have their own test (knife edges, fp64 referee); evaluation
    with discrete allocation against the oracle."""
    from oracle import inventory_oracle as orc
    assert len(TAPE_CASES) == 6
    g = Golden(name)
    c = g.fresh_config()
    model = _model(g, c)
    data = {k: v.to(DEV) for k, v in g.data.items()}
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    if g.params:
        obs, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
        with torch.no_grad():
            o = dict(obs)
            o["internal_data"] = sim._internal_data
            model(o)   # materialises the lazy layers
        _load(model, g)
    model.zero_grad()
    total, reported = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data,
                                        c["observation_params"], c["ignore"], False)
    eng = tr._last_engine
    assert type(eng).__name__ == "TapeRollout"
    assert total.requires_grad == (name in QUANTILE_TRAINABLE)
    torch.cuda.synchronize()
    assert abs(float(total) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))
    assert abs(float(reported) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
    torch.testing.assert_close(eng.per_period_rewards().cpu(), g.tensor("rewards").float(), rtol=1e-5, atol=2e-2)
    final = eng.final_state()
    for k, v in g.states(c["periods"]).items():
        torch.testing.assert_close(final[k].cpu(), v.float(), rtol=2e-6, atol=2e-3)
    if name in QUANTILE_TRAINABLE:   # the backward launch runs and reaches every parameter
        (total / (c["n"] * c["periods"])).backward()
        assert all(p_.grad is not None and bool(torch.isfinite(p_.grad).all()) for p_ in model.parameters())
    # evaluation: same numbers without the histories; discrete allocation (orders rounded half to even) against the oracle
    with torch.no_grad():
        t2, r2 = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data, c["observation_params"],
                                   c["ignore"], False)
        t3, r3 = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data, c["observation_params"],
                                   c["ignore"], True)
    assert float(t2) == float(total) and float(r2) == float(reported)
    pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"),
                                     forecaster_state=g.forecaster)
    with torch.no_grad():
        ref = orc.rollout(pol, c["periods"], c["problem_params"], g.data, c["observation_params"], c["ignore"],
                          discrete_allocation=True)
    assert abs(float(t3) - float(ref.total)) <= 1e-5 * abs(float(ref.total))
    assert abs(float(r3) - float(ref.reported)) <= 1e-5 * abs(float(ref.reported))


def test_tape_engine_refuses_the_backward_of_an_overwritten_rollout():
    """The whole-horizon adjoint reads histories that belong to the ENGINE: a backward through an older rollout, after the same
    engine has run again, would silently use the newer run's states - it raises instead; the usual order (forward, backward,
    forward, backward) works and gives the same gradients twice."""
    name = QUANTILE_TRAINABLE[1]
    g = Golden(name)
    c = g.fresh_config()
    model = _model(g, c)
    data = {k: v.to(DEV) for k, v in g.data.items()}
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    obs, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
    with torch.no_grad():
        o = dict(obs)
        o["internal_data"] = sim._internal_data
        model(o)
    _load(model, g)

    def run():
        return tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data, c["observation_params"],
                                 c["ignore"], False)[0]
    grads = []
    for _ in range(2):
        model.zero_grad()
        run().backward()
        grads.append([p_.grad.clone() for p_ in model.parameters()])
    for a, b in zip(*grads):   # (autograd's scatter-adds behind the interpolation are atomic: not bit-reproducible)
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    first = run()
    run()
    with pytest.raises(RuntimeError, match="overwritten"):
        first.backward()


@pytest.mark.parametrize("name", [n for n in case_names() if n.startswith("f4_real")])
def test_real_data_observations_and_dynamics_follow_the_reference_tape(name):
    """`Simulator.reset/step` on a real-data setting (period_shift 16, past-demand window of 16, days from
    christmas, profit objective) driven by the reference's own action tape: every period's observation features and state are
    the reference's, per-period rewards within 1e-5."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    sim = Simulator(device=DEV)
    obs, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
    ref_r = g.tensor("rewards").float()
    assert sim._internal_data["period_shift"] == c["observation_params"]["demand"]["period_shift"] == 16
    for t in range(c["periods"]):
        for k, v in g.features(t).items():
            assert torch.equal(obs[k].cpu(), v), (t, k)
        for k, v in g.states(t).items():
            torch.testing.assert_close(obs[k].cpu(), v.float(), rtol=2e-6, atol=2e-3)
        action = {k: v.float().to(DEV) for k, v in g.actions(t).items()}
        obs, reward, terminated, _, _ = sim.step(action)
        torch.testing.assert_close(reward.cpu(), ref_r[t], rtol=1e-5, atol=2e-2)
        assert bool(terminated) == (t == c["periods"] - 1)


@pytest.mark.parametrize("name", ["cfg1_one_store_lost_vanilla", "cfg3_one_warehouse_5_vanilla", "cfg4_serial_vanilla"])
def test_trainer_epoch_both_routes_agree_and_step(name):
    g = Golden(name)
    c = g.fresh_config()
    sc = Scenario(c["periods"], c["problem_params"], c["store_params"], c["warehouse_params"], c["echelon_params"],
                  c["n"], c["observation_params"], c["seeds"])
    ds = DatasetCreator().create_datasets(sc, split=False)
    losses = []
    for fused in (True, False):
        model = NeuralNetworkCreator().create_neural_network(sc, c["nn_params"], device=DEV)
        tr, sim = Trainer(device=DEV), Simulator(device=DEV)
        tr.use_fused_rollout = fused
        loader = DeviceBatches(ds, c["n"], shuffle=False, device=DEV)
        batch = next(iter(loader))
        obs, _ = sim.reset(c["periods"], c["problem_params"], batch, c["observation_params"])
        with torch.no_grad():
            o = dict(obs)
            o["internal_data"] = sim._internal_data
            model(o)
        _load(model, g)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        before = [p.detach().clone() for p in model.parameters()]
        out = tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"],
                              c["observation_params"], train=True, ignore_periods=c["ignore"])
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        losses.append(out)
        ref_avg = float(g.z["total"]) / (c["n"] * c["periods"] * c["problem_params"]["n_stores"])
        assert abs(out[0] - ref_avg) <= 1e-5 * abs(ref_avg)
        ev = tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"],
                             c["observation_params"], train=False, ignore_periods=c["ignore"])
        assert np.isfinite(ev[0]) and np.isfinite(ev[1])
    assert abs(losses[0][0] - losses[1][0]) <= 2e-6 * abs(losses[0][0])
    assert abs(losses[0][1] - losses[1][1]) <= 2e-6 * abs(losses[0][1])


def test_checkpoint_known_answer_through_hip():
    """The reference's shipped checkpoint (best dev loss 6.854347610473633) evaluated by the HIP engine."""
    g = Golden("checkpoint_kat")
    c = g.fresh_config()
    sc = Scenario(c["scenario_periods"], c["problem_params"], c["store_params"], None, None, c["scenario_samples"],
                  c["observation_params"], c["seeds"])
    _, dev_ds = DatasetCreator().create_datasets(sc, split=True, by_sample_indexes=True,
                                                 sample_index_for_split=c["dev_samples"])
    model = NeuralNetworkCreator().create_neural_network(sc, c["nn_params"], device=DEV)
    tr, sim = Trainer(device=DEV), Simulator(device=DEV)
    materialize_linears(model.master_linears(), 4)
    model.load_state_dict({k: v.to(DEV) for k, v in g.params.items()})
    loader = DeviceBatches(dev_ds, c["dev_samples"], device=DEV)
    for fused in (True, False):
        tr.use_fused_rollout = fused
        _, report = tr.do_one_epoch(None, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"],
                                    c["observation_params"], train=False, ignore_periods=c["ignore"])
        assert abs(report - 6.854347610473633) < 2e-6, (fused, report)


def test_full_size_properties_cfg3():
    """BASELINE cfg3 shape (65,536 scenarios x 16 stores), short horizon: (1) every scenario's trajectory is independent
    of the batch it sits in (bit-exact vs a 24-scenario run of the same scenarios); (2) lost-demand stock conservation:
    sum(store pipelines)_{t+1} = sum_t - sales + orders received, sales = min(on hand, demand)."""
    g = Golden("cfg3_one_warehouse_16_vanilla")
    c = g.fresh_config()
    B, T = 65536, 6
    model = _model(g, c)
    eng = FusedRollout(model, c["problem_params"], DEV)
    eng.materialize(16 * 3 + 3)
    _load(model, g)
    small = {k: v.to(DEV) for k, v in g.data.items()}
    n = c["n"]
    reps = B // n + 1
    big = {k: v.repeat(*([reps] + [1] * (v.dim() - 1)))[:B].contiguous() for k, v in small.items()}
    gen = torch.Generator(device="cpu").manual_seed(1)
    big["demands"][n:] = (torch.rand(B - n, 16, c["periods"], generator=gen) * 10).to(DEV)
    eng.run(big, T, 0, train=False, observation_params=c["observation_params"])
    r_big = eng.per_period_rewards()[:, :n].clone()
    states = eng.states.clone()
    orders = eng.orders.clone()
    eng_s = FusedRollout(model, c["problem_params"], DEV)
    eng_s.fuse_tail = False   # (the same launches as the full batch: bit for bit)
    eng_s.run(small, T, 0, train=False, observation_params=c["observation_params"])
    assert torch.equal(eng_s.per_period_rewards(), r_big)
    # round 5: a batch this small takes the fused tail launches by default (another association of the same products in the
    # logits contraction, the first layer's bias inside its contraction): fp32 round-off of the per-period cost
    eng_t = FusedRollout(model, c["problem_params"], DEV)
    eng_t.run(small, T, 0, train=False, observation_params=c["observation_params"])
    assert eng_t._use_tail() and not eng._use_tail()
    torch.testing.assert_close(eng_t.per_period_rewards(), r_big, rtol=2e-6, atol=1e-4)
    # conservation over all 65,536 scenarios
    S, Ws = 16, 3
    for t in range(T):
        st = states[t][:S * Ws].view(S, Ws, -1)[:, :, :B].double()
        nx = states[t + 1][:S * Ws].view(S, Ws, -1)[:, :, :B].double()
        dem = eng.demand[t][:, :B].double()
        sales = torch.minimum(st[:, 0], dem)
        recv = orders[t][:S].view(S, -1)[:, :B].double()
        lhs = nx.sum(dim=1)
        rhs = st.sum(dim=1) - sales + recv
        assert float((lhs - rhs).abs().max()) < 1e-3


@pytest.mark.parametrize("name", ["cfg2_one_store_backlogged_vanilla", "cfg4_serial_vanilla", "cfg3_one_warehouse_5_vanilla",
                                  "cfg5_many_warehouses_3x64_vanilla"])   # (the last one: compacted logits layer, row copies)
@pytest.mark.parametrize("tail", [True, False])
def test_graph_replay_matches_eager(name, tail):
    """HIP-graph replay of the launch sequence (use_graph) is bit-identical to eager launches, also after the batch
    contents change between calls (the captured graph points at engine-owned buffers that are refreshed per call).
    `tail`: the fused per-period tail launches forced on (both directions, where the shapes qualify) / off - under "auto" the
    engine picks the backward tail by batch size AND replay mode, so eager and replayed runs may legitimately sum the logits
    layer's weight gradient in different orders."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    data2 = dict(data)
    data2["demands"] = (data["demands"] * 1.25 + 0.5).contiguous()
    data2["initial_inventories"] = (data["initial_inventories"] * 0.5).contiguous()
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if c["policy"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)
    results = {}
    for mode in ("eager", "graph"):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.use_graph = mode == "graph"
        eng.fuse_tail = tail
        eng.use_small = False  # the whole-horizon route is three launches; graphs matter for the per-period route
        eng.materialize(F)
        _load(model, g)
        out = []
        for d in (data, data2, data, data2):  # call 1 eager, call 2 captures, calls 3-4 replay
            total, rep = eng.run(d, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
            torch.cuda.synchronize()
            out.append((float(total), float(rep), [p.grad.clone() for p in model.parameters()],
                        eng.per_period_rewards().clone()))
        results[mode] = out
        if mode == "graph":
            assert set(eng._graphs) == {"fwd", "bwd"}
    for a, b in zip(results["eager"], results["graph"]):
        assert a[0] == b[0] and a[1] == b[1]
        assert torch.equal(a[3], b[3])
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x, y)
    assert results["eager"][0][0] != results["eager"][1][0]  # the two batches really differ
    assert results["eager"][0][0] == results["eager"][2][0]


def test_trainer_train_loop_checkpoint_and_test(tmp_path):
    """Trainer.train end to end on the HIP path (reference signature, trainer.py:29-119): loss goes down, the best
    parameters are tracked, a checkpoint with the reference's dict keys is written and loads back, test() runs."""
    from neural_inventory_control_amd import workloads
    from collections import defaultdict
    setting, policy, _, _, _ = workloads.get("cfg2")
    obs = defaultdict(lambda: None, setting["observation_params"])
    n_train, n_dev, T = 512, 256, 30
    sc = Scenario(T, setting["problem_params"], setting["store_params"], None, None, n_train + n_dev, obs, setting["seeds"])
    train_ds, dev_ds = DatasetCreator().create_datasets(sc, split=True, by_sample_indexes=True, sample_index_for_split=n_dev)
    loaders = {"train": DeviceBatches(train_ds, 256, shuffle=True, device=DEV, seed=1),
               "dev": DeviceBatches(dev_ds, 256, device=DEV), "test": DeviceBatches(dev_ds, 256, device=DEV)}
    torch.manual_seed(0)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    tr, sim = Trainer(device=DEV), Simulator(device=DEV)
    pbd = {k: {"periods": T, "ignore_periods": 10} for k in ("train", "dev", "test")}
    tp = {"do_dev_every_n_epochs": 5, "print_results_every_n_epochs": 1000, "save_model": True, "epochs_between_save": 1,
          "choose_best_model_on": "dev_loss", "early_stopping_patience_epochs": 1000, "base_dir": str(tmp_path),
          "save_model_folders": ["a", "b"], "save_model_filename": "ckpt"}
    tr.train(40, PolicyLoss(), sim, model, loaders, opt, setting["problem_params"], obs, pbd, tp)
    assert len(tr.all_train_losses) == 40 and len(tr.all_dev_losses) == 40
    assert tr.all_train_losses[-1] < 0.7 * tr.all_train_losses[0]
    assert tr.best_performance_data["dev_loss"] < tr.all_dev_losses[0]
    ck = torch.load(tmp_path / "a" / "b" / "ckpt.pt", map_location="cpu", weights_only=False)
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "best_train_loss", "best_dev_loss", "all_train_losses",
            "all_dev_losses", "all_test_losses", "warehouse_upper_bound"} <= set(ck)
    model2 = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    materialize_linears(model2.master_linears(), 4)
    opt2 = torch.optim.Adam(model2.parameters(), lr=3e-3)
    tr2 = Trainer(device=DEV)
    tr2.load_model(model2, opt2, str(tmp_path / "a" / "b" / "ckpt.pt"))
    best = tr.best_performance_data["model_params_to_save"]
    for k, v in model2.state_dict().items():
        assert torch.equal(v, best[k])
    _, rep = tr.test(PolicyLoss(), sim, model, loaders, opt, setting["problem_params"], obs, pbd)
    assert abs(rep - tr.best_performance_data["dev_loss"]) < 1e-4 * abs(rep)
    # resume into a FUSED Adam (what main_run builds on a GPU, main_run.py:110) and into a default one, then train on: the fused
    # one needs its `step` counters on the device, the default one on the host; both must take the same steps
    after = {}
    for kind, kw in (("fused", {"fused": True}), ("default", {})):
        model3 = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        materialize_linears(model3.master_linears(), 4)
        opt3 = torch.optim.Adam(model3.parameters(), lr=3e-3, **kw)
        tr3 = Trainer(device=DEV)
        tr3.load_model(model3, opt3, str(tmp_path / "a" / "b" / "ckpt.pt"))
        for g in opt3.param_groups:
            assert bool(g.get("fused")) == (kind == "fused")
            for p in g["params"]:
                step = opt3.state[p]["step"]
                assert (step.device == p.device) == (kind == "fused"), (kind, step.device)
                assert float(step) > 0
        loaders3 = {"train": DeviceBatches(train_ds, 256, shuffle=True, device=DEV, seed=7)}
        tr3.do_one_epoch(opt3, loaders3["train"], PolicyLoss(), sim, model3, T, setting["problem_params"], obs, train=True,
                         ignore_periods=10)
        torch.cuda.synchronize()
        after[kind] = [p.detach().clone() for p in model3.parameters()]
        assert all(torch.isfinite(p).all() for p in after[kind])
    for a, b in zip(after["fused"], after["default"]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", ["cfg1_one_store_lost_vanilla", "cfg2_one_store_backlogged_vanilla", "cfg4_serial_vanilla"])
def test_small_rollout_kernels_match_reference(name):
    """Whole-horizon kernels (nic_small_rollout_fwd/bwd through the C ABI) against the reference's golden vectors."""
    import small_rollout_checks as src
    from neural_inventory_control_amd import small_rollout as sr
    out = src.run_case(name, sr.small_rollout_fwd,
                       lambda d, sh, hh, lh, gr, dzh, dzo: _lib.check(_lib.lib().nic_small_rollout_bwd(
                           d, sh.data_ptr(), hh.data_ptr(), lh.data_ptr(), gr, dzh.data_ptr(), dzo.data_ptr(),
                           _lib.current_stream())),
                       DEV, sync=torch.cuda.synchronize)
    assert out["worst"] <= GRAD_TOL


@pytest.mark.parametrize("workload,n,T", [("cfg2", 1000, 23), ("cfg4", 333, 17), ("cfg1", 70, 9)])
def test_small_route_in_kernel_weight_gradients_match_the_gemm_path(workload, n, T):
    """The whole-horizon backward contracts the weight gradients itself (one partial gradient per wavefront, summed once); the
    first version wrote a dZ history and ran one GEMM per layer over it.  Same gradients on ragged batches (scenario counts
    that leave dead lanes in the last wavefront, which shadow scenario 0 and must not be counted)."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.rollout import KernelTimer
    setting, policy, _, _, _ = workloads.get(workload)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, setting["seeds"])
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    res = {}
    # (in-kernel weight gradients with 16 scenarios per wavefront - the engine's default -, with 32, and the dz-history path)
    for in_kernel, width in ((True, 16), (True, 32), (False, 32)):
        torch.manual_seed(5)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng = FusedRollout(model, setting["problem_params"], DEV)
        eng.small_wgrad_in_kernel = in_kernel
        eng.small_lane_scenarios = width
        F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
        if policy["name"] != "vanilla_one_store":
            F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                     if k in data)
        eng.materialize(F)
        eng.timer = KernelTimer()   # (records which kernel the C ABI launched for every class of the step)
        total, _ = eng.run(data, T, 0, train=True, observation_params=obs)
        torch.cuda.synchronize()
        assert eng.small is not None
        for tag in ("small_rollout_fwd", "small_rollout_bwd"):
            assert ("small_rollout16" in eng.timer.names[tag]) == (width == 16), eng.timer.names
        res[(in_kernel, width)] = (float(total), [p.grad.clone() for p in model.parameters()])
    ref = res[(False, 32)]
    assert res[(True, 32)][0] == ref[0]   # same forward kernel
    assert abs(res[(True, 16)][0] - ref[0]) <= 2e-6 * abs(ref[0])
    for key in ((True, 16), (True, 32)):
        for x, y in zip(res[key][1], ref[1]):
            assert float((x - y).norm() / (y.norm() + 1e-30)) < 5e-6, key


@pytest.mark.parametrize("variant", ["one_store_ws3", "serial_one_echelon", "serial_ww4"])
def test_small_route_run_time_structure_kernels_match_the_per_period_route(variant):
    """The whole-horizon kernels are compiled with the structure of the two chains the reference ships as constants; every other
    supported chain takes the run-time-structure instantiation.  Three such chains (store pipeline of 3 slots; store + warehouse +
    ONE echelon; a 4-slot warehouse pipeline) against the engine's own per-period route: costs, final state, gradients."""
    from collections import defaultdict
    import copy
    from neural_inventory_control_amd import workloads
    if variant == "one_store_ws3":
        setting, policy, _, _, _ = workloads.get("cfg2")
        setting = copy.deepcopy(setting)
        setting["store_params"]["lead_time"] = {"sample_across_stores": False, "vary_across_samples": False, "expand": True, "value": 3}
        setting["store_params"]["initial_inventory"]["inventory_periods"] = 3
    else:
        setting, policy, _, _, _ = workloads.get("cfg4")
        setting, policy = copy.deepcopy(setting), copy.deepcopy(policy)
        if variant == "serial_one_echelon":
            setting["problem_params"]["n_extra_echelons"] = 1
            setting["echelon_params"] = {"holding_cost": [0.1], "lead_time": [3]}
            policy["output_sizes"]["master"] = 3   # one sigmoid head per echelon + warehouse + store
        else:
            setting["warehouse_params"] = {"holding_cost": 0.5, "lead_time": 4}
    obs = defaultdict(lambda: None, setting["observation_params"])
    n, T = 333, 13
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, setting["seeds"])
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if policy["name"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)
    res = {}
    for small in (True, False):
        torch.manual_seed(9)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng = FusedRollout(model, setting["problem_params"], DEV)
        eng.use_small = small
        eng.materialize(F)
        total, rep = eng.run(data, T, 3, train=True, observation_params=obs)
        torch.cuda.synchronize()
        assert (eng.small is not None) == small
        res[small] = (float(total), float(rep), [p.grad.clone() for p in model.parameters()],
                      {k: v.clone() for k, v in eng.final_state().items()})
    a, b = res[True], res[False]
    assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2e-6 * abs(b[1])
    for x, y in zip(a[2], b[2]):
        assert float((x - y).norm() / (y.norm() + 1e-30)) < GRAD_TOL
    for k in b[3]:
        torch.testing.assert_close(a[3][k], b[3][k], **STATE_TOL)


# What the whole-horizon route records for the two compiled-in chains (cfg2: one store, cfg4: serial) at every depth, literally:
# (workload, hidden layers, mode) -> (small_rollout_fwd, small_rollout_bwd); modes: in-kernel weight gradients at 16 and at 32 scenarios
# per wavefront, and the dz-history backward (32 only).  A name states the request; which instantiation runs it is
# csrc/small_rollout_variants.h's decision (tests/test_small_rollout_variants_host.py), and a wrong one shows in the numbers below.
SMALL_DISPATCH_KERNELS = {
    ("cfg2", 1, "wgrad16"): ("small_rollout16_fwd_kernel<1,one_store>", "small_rollout16_bwd_kernel<1,wgrad,one_store>"),
    ("cfg2", 1, "wgrad32"): ("small_rollout_fwd_mfma_kernel<1,one_store>", "small_rollout_bwd_mfma_kernel<1,wgrad,one_store>"),
    ("cfg2", 1, "dz32"): ("small_rollout_fwd_mfma_kernel<1,one_store>", "small_rollout_bwd_mfma_kernel<1,one_store>"),
    ("cfg2", 2, "wgrad16"): ("small_rollout16_fwd_kernel<2,one_store>", "small_rollout16_bwd_kernel<2,wgrad,one_store>"),
    ("cfg2", 2, "wgrad32"): ("small_rollout_fwd_mfma_kernel<2,one_store>", "small_rollout_bwd_mfma_kernel<2,wgrad,one_store>"),
    ("cfg2", 2, "dz32"): ("small_rollout_fwd_mfma_kernel<2,one_store>", "small_rollout_bwd_mfma_kernel<2,one_store>"),
    ("cfg2", 3, "wgrad16"): ("small_rollout16_fwd_kernel<3,one_store>", "small_rollout16_bwd_kernel<3,wgrad,one_store>"),
    ("cfg2", 3, "wgrad32"): ("small_rollout_fwd_mfma_kernel<3,one_store>", "small_rollout_bwd_mfma_kernel<3,wgrad,one_store>"),
    ("cfg2", 3, "dz32"): ("small_rollout_fwd_mfma_kernel<3,one_store>", "small_rollout_bwd_mfma_kernel<3,one_store>"),
    ("cfg4", 1, "wgrad16"): ("small_rollout16_fwd_kernel<1,serial>", "small_rollout16_bwd_kernel<1,wgrad,serial>"),
    ("cfg4", 1, "wgrad32"): ("small_rollout_fwd_mfma_kernel<1,serial>", "small_rollout_bwd_mfma_kernel<1,wgrad,serial>"),
    ("cfg4", 1, "dz32"): ("small_rollout_fwd_mfma_kernel<1,serial>", "small_rollout_bwd_mfma_kernel<1,serial>"),
    ("cfg4", 2, "wgrad16"): ("small_rollout16_fwd_kernel<2,serial>", "small_rollout16_bwd_kernel<2,wgrad,serial>"),
    ("cfg4", 2, "wgrad32"): ("small_rollout_fwd_mfma_kernel<2,serial>", "small_rollout_bwd_mfma_kernel<2,wgrad,serial>"),
    ("cfg4", 2, "dz32"): ("small_rollout_fwd_mfma_kernel<2,serial>", "small_rollout_bwd_mfma_kernel<2,serial>"),
    ("cfg4", 3, "wgrad16"): ("small_rollout16_fwd_kernel<3,serial>", "small_rollout16_bwd_kernel<3,wgrad,serial>"),
    ("cfg4", 3, "wgrad32"): ("small_rollout_fwd_mfma_kernel<3,serial>", "small_rollout_bwd_mfma_kernel<3,wgrad,serial>"),
    ("cfg4", 3, "dz32"): ("small_rollout_fwd_mfma_kernel<3,serial>", "small_rollout_bwd_mfma_kernel<3,serial>"),
}


@pytest.mark.parametrize("n_hidden", [1, 2, 3])
@pytest.mark.parametrize("workload", ["cfg2", "cfg4"])
def test_small_route_dispatch_cells_match_the_per_period_route(workload, n_hidden):
    """Every (chain, depth) cell of the whole-horizon kernels' dispatch through the engine, in the three modes that reach different
    kernels, against the engine's own per-period route: recorded kernel names, costs, gradients, final state.  40 scenarios (three
    16-scenario wavefronts or two 32-scenario ones, the last ragged), 5 periods."""
    from collections import defaultdict
    import copy
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.rollout import KernelTimer
    setting, policy, _, _, _ = workloads.get(workload)
    policy = copy.deepcopy(policy)
    policy["neurons_per_hidden_layer"]["master"] = [32] * n_hidden
    obs = defaultdict(lambda: None, setting["observation_params"])
    n, T = 40, 5
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, setting["seeds"])
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if policy["name"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)

    def run(mode):
        torch.manual_seed(9)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng = FusedRollout(model, setting["problem_params"], DEV)
        eng.use_small = mode != "periods"
        if mode != "periods":
            eng.small_wgrad_in_kernel = mode != "dz32"
            eng.small_lane_scenarios = 16 if mode == "wgrad16" else 32
        eng.materialize(F)
        eng.timer = KernelTimer()   # (records which kernel the C ABI launched for every class of the step)
        total, rep = eng.run(data, T, 2, train=True, observation_params=obs)
        torch.cuda.synchronize()
        assert (eng.small is not None) == (mode != "periods")
        assert len(eng._linears()) == n_hidden + 1
        names = (eng.timer.names.get("small_rollout_fwd"), eng.timer.names.get("small_rollout_bwd"))
        return (float(total), float(rep), [p.grad.clone() for p in model.parameters()],
                {k: v.clone() for k, v in eng.final_state().items()}), names
    b, names = run("periods")
    assert names == (None, None)
    for mode in ("wgrad16", "wgrad32", "dz32"):
        a, names = run(mode)
        assert names == SMALL_DISPATCH_KERNELS[workload, n_hidden, mode], mode
        assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2e-6 * abs(b[1]), mode
        for x, y in zip(a[2], b[2]):
            assert float((x - y).norm() / (y.norm() + 1e-30)) < GRAD_TOL, mode
        for k in b[3]:
            torch.testing.assert_close(a[3][k], b[3][k], **STATE_TOL)


@pytest.mark.parametrize("name", ["cfg2_one_store_backlogged_vanilla", "cfg4_serial_vanilla"])
def test_small_route_equals_per_period_route(name):
    """FusedRollout takes the whole-horizon route for these policies; it must agree with its own per-period route."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if c["policy"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)
    res = {}
    for small in (True, False):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.use_small = small
        eng.materialize(F)
        _load(model, g)
        total, rep = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
        torch.cuda.synchronize()
        assert (eng.small is not None) == small
        res[small] = (float(total), float(rep), eng.per_period_rewards().clone(), [p.grad.clone() for p in model.parameters()],
                      {k: v.clone() for k, v in eng.final_state().items()})
    a, b = res[True], res[False]
    assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2e-6 * abs(b[1])
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-4)
    for x, y in zip(a[3], b[3]):
        assert float((x - y).norm() / (y.norm() + 1e-30)) < GRAD_TOL
    for k in b[4]:
        torch.testing.assert_close(a[4][k], b[4][k], **STATE_TOL)


@pytest.mark.parametrize("name", ["cfg3_one_warehouse_16_vanilla", "cfg5_many_warehouses_2x10_vanilla"])
def test_fused_thin_layer_backward_equals_separate_gemms(name):
    """The logits layer's backward runs as one fused pass (nic_linear_bwd_thin); switching it off must give the same
    gradients through nic_linear_wgrad + nic_linear_dgrad."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    F = sum(int(np.prod(data[k].shape[1:])) for k in ("initial_inventories", "initial_warehouse_inventories") if k in data)
    res = {}
    for thin in (True, False):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.use_thin = thin
        eng.fuse_tail = False   # (the separate launches are what this test compares)
        eng.materialize(F)
        _load(model, g)
        total, _ = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
        torch.cuda.synchronize()
        assert any(eng._thin) == thin
        res[thin] = (float(total), [p.grad.clone() for p in model.parameters()])
    assert res[True][0] == res[False][0]
    for x, y in zip(res[True][1], res[False][1]):
        assert float((x - y).norm() / (y.norm() + 1e-30)) < GRAD_TOL


@pytest.mark.parametrize("name", ["cfg3_one_warehouse_16_vanilla", "cfg5_many_warehouses_3x8_vanilla"])
def test_batched_weight_gradients_equal_per_period_contraction(name):
    """Hidden-layer weight gradients are contracted over all periods in one launch (nic_linear_wgrad_periods); with that
    switched off the engine accumulates them period by period — same gradients."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    F = sum(int(np.prod(data[k].shape[1:])) for k in ("initial_inventories", "initial_warehouse_inventories") if k in data)
    res = {}
    for batched in (True, False):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.batch_wgrad = batched
        eng.materialize(F)
        _load(model, g)
        total, _ = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
        torch.cuda.synchronize()
        assert (eng.dZhist is not None) == batched
        res[batched] = (float(total), [p.grad.clone() for p in model.parameters()])
    assert res[True][0] == res[False][0]
    for x, y in zip(res[True][1], res[False][1]):
        assert float((x - y).norm() / (y.norm() + 1e-30)) < GRAD_TOL


@pytest.mark.parametrize("name,B", [("cfg3_one_warehouse_16_vanilla", 333), ("cfg1_one_store_lost_vanilla", 201),
                                     ("cfg4_serial_vanilla", 130), ("cfg5_many_warehouses_2x10_vanilla", 77)])
def test_ragged_multi_block_batch_matches_oracle(name, B):
    """Batch sizes that are neither a multiple of 4 nor of the 64-scenario block (several blocks + a ragged tail), fresh
    random demands: per-scenario costs, totals and gradients of the HIP engine against the CPU oracle on the same inputs."""
    from oracle import inventory_oracle as orc
    g = Golden(name)
    c = g.fresh_config()
    n = c["n"]
    reps = B // n + 1
    gen = torch.Generator(device="cpu").manual_seed(B)
    data = {k: v.repeat(*([reps] + [1] * (v.dim() - 1)))[:B].contiguous() for k, v in g.data.items()}
    d = data["demands"]
    data["demands"] = (d * (0.5 + torch.rand(d.shape, generator=gen))).contiguous()
    model = _model(g, c)
    eng = FusedRollout(model, c["problem_params"], DEV)
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if c["policy"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)
    eng.materialize(F)
    _load(model, g)
    total, reported = eng.run({k: v.to(DEV) for k, v in data.items()}, c["periods"], c["ignore"], train=True,
                              observation_params=c["observation_params"])
    torch.cuda.synchronize()
    pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"))
    res, _, grads = orc.train_step_gradients(pol, c["periods"], c["problem_params"], data, c["observation_params"],
                                             c["ignore"])
    assert abs(float(total) - float(res.total)) <= 1e-5 * abs(float(res.total))
    assert abs(float(reported) - float(res.reported)) <= 1e-5 * abs(float(res.reported))
    tot_b = eng.per_period_rewards().sum(dim=0).cpu()
    ref_b = res.per_period.sum(dim=0)
    assert float(((tot_b - ref_b).abs() / ref_b.abs().clamp_min(1e-9)).max()) <= 1e-5
    for p, ref in zip(model.parameters(), grads):
        assert _rel(p.grad, ref) <= GRAD_TOL


# ---- evaluation (Trainer.test): forward only, discrete allocation, long horizons -----------------------

@pytest.mark.parametrize("name", ["cfg1_one_store_lost_vanilla", "cfg4_serial_vanilla", "cfg3_one_warehouse_16_vanilla",
                                  "cfg5_many_warehouses_2x10_vanilla"])
@pytest.mark.parametrize("rolling", [False, True])
def test_discrete_allocation_evaluation_matches_oracle(name, rolling):
    """`Trainer.test` with discrete allocation (trainer.py:201-202: actions rounded half to even before the env step), with
    the per-period history kept and with the rolling two-block state buffer a long-horizon evaluation uses."""
    from oracle import inventory_oracle as orc
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    model = _model(g, c)
    eng = FusedRollout(model, c["problem_params"], DEV)
    eng.eval_history = not rolling
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    if c["policy"] != "vanilla_one_store":
        F += sum(int(np.prod(data[k].shape[1:])) for k in ("initial_warehouse_inventories", "initial_echelon_inventories")
                 if k in data)
    eng.materialize(F)
    _load(model, g)
    with torch.no_grad():
        total, reported = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"],
                                  discrete_allocation=True)
    torch.cuda.synchronize()
    pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"))
    with torch.no_grad():
        res = orc.rollout(pol, c["periods"], c["problem_params"], g.data, c["observation_params"], c["ignore"],
                          discrete_allocation=True)
    assert abs(float(total) - float(res.total)) <= 1e-5 * abs(float(res.total))
    assert abs(float(reported) - float(res.reported)) <= 1e-5 * abs(float(res.reported))
    torch.testing.assert_close(eng.per_period_rewards().cpu(), res.per_period, rtol=1e-5, atol=1e-4)
    final = eng.final_state()
    for k, v in res.final_obs.items():
        if k in final:
            torch.testing.assert_close(final[k].cpu(), v, **STATE_TOL)
    # rounding changes the trajectory: the continuous evaluation gives a different cost
    t_cont, _ = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
    assert float(t_cont) != float(total)
    with pytest.raises(ValueError):
        eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"],
                discrete_allocation=True)


def test_long_horizon_evaluation_matches_oracle():
    """one_store_lost + vanilla_one_store, Poisson demand, discrete allocation, T = 5000 periods (the reference's test
    horizon, one_store_lost.yml:43-44) on 256 scenarios: whole-horizon kernel against the oracle's period loop."""
    from oracle import inventory_oracle as orc
    g = Golden("cfg1_one_store_lost_vanilla")
    c = g.fresh_config()
    B, T, ignore = 256, 5000, 3000
    gen = torch.Generator().manual_seed(7)
    data = {k: v.repeat(*([B // c["n"] + 1] + [1] * (v.dim() - 1)))[:B].contiguous() for k, v in g.data.items()}
    data["demands"] = torch.poisson(torch.full((B, 1, T), 5.0), generator=gen)
    model = _model(g, c)
    eng = FusedRollout(model, c["problem_params"], DEV)
    eng.materialize(data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2])
    _load(model, g)
    with torch.no_grad():
        total, reported = eng.run({k: v.to(DEV) for k, v in data.items()}, T, ignore, train=False,
                                  observation_params=c["observation_params"], discrete_allocation=True)
        pol = orc.policy_from_state_dict(c["nn_params"], g.params, c["problem_params"], g.tensor("warehouse_upper_bound"))
        res = orc.rollout(pol, T, c["problem_params"], data, c["observation_params"], ignore, discrete_allocation=True)
    # a rounding knife edge (x.5 +- 1 ulp) may differ in a handful of the 1.28 M actions: compare aggregate costs
    assert abs(float(total) - float(res.total)) <= 1e-5 * abs(float(res.total))
    assert abs(float(reported) - float(res.reported)) <= 1e-5 * abs(float(res.reported))
    per_scn = (eng.per_period_rewards().sum(dim=0).cpu() - res.per_period.sum(dim=0)).abs() / res.per_period.sum(dim=0)
    frac = float((per_scn <= 1e-5).float().mean())
    print(f"T=5000 discrete evaluation: {frac:.4f} of {B} scenarios within 1e-5 of the oracle; worst {float(per_scn.max()):.2e}")
    assert frac >= 0.99, f"only {frac:.4f} of the scenarios within 1e-5 (worst {float(per_scn.max()):.2e})"


def _one_store_yaml_dicts(tmp_path):
    """A full pair of config dicts in the reference's YAML schema (settings/one_store_lost.yml +
    policies_and_hyperparams/vanilla_one_store.yml shape), scaled down."""
    from neural_inventory_control_amd import workloads
    setting, policy, _, _, _ = workloads.get("cfg1")
    setting = dict(setting)
    setting["test_seeds"] = {k: v + 1 for k, v in setting["seeds"].items()}
    setting["params_by_dataset"] = {"train": {"n_samples": 256, "batch_size": 128, "periods": 20, "ignore_periods": 4},
                                    "dev": {"n_samples": 128, "batch_size": 128, "periods": 20, "ignore_periods": 4},
                                    "test": {"n_samples": 128, "batch_size": 128, "periods": 60, "ignore_periods": 20}}
    setting["sample_data_params"] = {"split_by_period": False}
    hyper = {"trainer_params": {"epochs": 3, "do_dev_every_n_epochs": 1, "print_results_every_n_epochs": 100,
                                "save_model": True, "epochs_between_save": 1, "choose_best_model_on": "dev_loss",
                                "load_previous_model": False, "load_model_path": "", "base_dir": str(tmp_path)},
             "optimizer_params": {"learning_rate": 0.01}, "nn_params": policy}
    return setting, hyper


def test_main_run_driver_trains_tests_and_saves(tmp_path, capsys):
    """The reference's `main_run.py train <setting> <hyperparams>` flow through the thin driver: datasets -> device batches
    -> policy -> Trainer.train (dev pass, best-model copy, checkpoint) -> Trainer.test with discrete allocation (Poisson)."""
    import glob
    import yaml
    from neural_inventory_control_amd import main_run
    setting, hyper = _one_store_yaml_dicts(tmp_path)
    (tmp_path / "settings").mkdir()
    (tmp_path / "policies_and_hyperparams").mkdir()
    (tmp_path / "settings" / "tiny_one_store.yml").write_text(yaml.safe_dump(setting))
    (tmp_path / "policies_and_hyperparams" / "tiny_vanilla.yml").write_text(yaml.safe_dump(hyper))
    main_run.main(["train", "tiny_one_store", "tiny_vanilla", "--config-dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert "Average per-period test loss:" in out
    loss = float(out.strip().split("Average per-period test loss:")[-1])
    assert 0.0 < loss < 1e4  # (three epochs on 256 scenarios: only sanity, the policy has barely moved)
    saved = glob.glob(str(tmp_path / "*" / "vanilla_one_store" / "*.pt"))
    assert len(saved) == 1
    ck = torch.load(saved[0], map_location="cpu", weights_only=False)
    assert {"model_state_dict", "optimizer_state_dict", "all_dev_losses", "warehouse_upper_bound"} <= set(ck)
    assert 1 <= len(ck["all_dev_losses"]) <= 3  # written at the last epoch whose dev loss improved
    assert ck["all_dev_losses"][-1] <= ck["all_dev_losses"][0]
    # `test` mode from the saved checkpoint reproduces a finite loss through the fused evaluation path
    hyper["trainer_params"].update(load_previous_model=True, load_model_path=saved[0])
    rep = main_run.run("test", setting, hyper)
    assert abs(rep - loss) <= 1e-6 * loss  # same best-dev parameters, same test set
    with pytest.raises(ValueError):
        main_run.run("deploy", setting, hyper)


@pytest.mark.parametrize("name,fused", [("f1_one_warehouse_gnn", False), ("cfg2_one_store_backlogged_capped", False),
                                        ("cfg4_serial_echelon_stock", False), ("cfg2_one_store_backlogged_capped", True),
                                        ("cfg2_one_store_backlogged_base_stock", True), ("cfg4_serial_echelon_stock", True)])
def test_captured_generic_training_step_matches_eager(name, fused):
    """Policies on the generic route (GNN, closed-form): the whole training step of a batch - every period's policy and
    env-step launches plus the autograd sweep - captured into one HIP graph (Trainer.use_step_graph) gives the same loss
    and gradients as eager execution, also after the batch contents change."""
    from neural_inventory_control_amd.environment import Simulator
    from neural_inventory_control_amd.loss_functions import PolicyLoss
    from neural_inventory_control_amd.trainer import Trainer
    g = Golden(name)
    c = g.fresh_config()
    base = {k: v.to(DEV) for k, v in g.data.items()}
    gen = torch.Generator().manual_seed(3)
    batches = [base]
    for _ in range(2):
        b = dict(base)
        b["demands"] = (base["demands"].cpu() * (0.5 + torch.rand(base["demands"].shape, generator=gen))).to(DEV)
        batches.append(b)

    def run(graph):
        model = _model(g, c)
        with torch.no_grad():  # materialise lazy layers, then load the fixture's weights
            sim0 = Simulator(device=DEV)
            obs0, _ = sim0.reset(c["periods"], c["problem_params"], dict(base), c["observation_params"])
            o = dict(obs0)
            o["internal_data"] = sim0._internal_data
            model(o)
        _load(model, g)
        tr = Trainer(device=DEV)
        tr.use_step_graph = graph
        # fused = False: the GENERIC route (one env-step launch per period + autograd); fused = True: the closed-form policies'
        # whole-horizon kernel - its launch, the tiny level network's autograd and the totals, all inside the captured step
        tr.use_fused_rollout = fused
        tr._global_batch = c["n"]
        sim, lf = Simulator(device=DEV), PolicyLoss()
        out = []
        for b in batches + batches[:1]:
            for p in model.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            if graph:
                total, rep = tr._graphed_generic_step(lf, sim, model, c["periods"], c["problem_params"], dict(b),
                                                      c["observation_params"], c["ignore"])
            else:
                total, rep = tr.simulate_batch(lf, sim, model, c["periods"], c["problem_params"], dict(b),
                                               c["observation_params"], c["ignore"], False)
                (total / (c["n"] * c["periods"] * c["problem_params"]["n_stores"])).backward()
            torch.cuda.synchronize()
            out.append((float(total), float(rep), [p.grad.clone() for p in model.parameters() if p.grad is not None]))
        return out

    eager, graphed = run(False), run(True)
    assert len(eager) == len(graphed) == 4
    for (te, re_, ge), (tg, rg, gg) in zip(eager, graphed):
        assert abs(te - tg) <= 1e-6 * abs(te) and abs(re_ - rg) <= 1e-6 * abs(re_)
        assert len(ge) == len(gg)
        for a, b2 in zip(ge, gg):
            assert float((a - b2).norm()) <= 1e-5 * float(a.norm()) + 1e-12


def test_gradient_parity_at_benchmark_width_and_horizon():
    """BASELINE cfg3's network (512 x 3) and horizon (T = 100) on 2,048 scenarios: the HIP engine's training step — weight
    gradients contracted over all 100 periods x 2,048 scenarios in one fp32 accumulation — against the CPU oracle's autograd
    on identical inputs and weights.  Per-scenario total cost: 1e-5 relative (north star).  Gradients: each side sums ~200k
    fp32 terms per weight in its own order, so the criterion is an fp64 REFEREE (the oracle evaluated in float64): per
    parameter tensor the engine must be no further from it than twice the reference's own float32 arithmetic is."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
    from oracle import inventory_oracle as orc
    torch.set_num_threads(min(32, torch.get_num_threads()))
    setting, policy, _, _, _ = workloads.get("cfg3")
    B, T = 2048, 100
    obs = defaultdict(lambda: None, setting["observation_params"])
    data = orc.generate_scenario_data(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"],
                                      setting["echelon_params"], B, obs, setting["seeds"])
    F = 16 * data["initial_inventories"].shape[2] + data["initial_warehouse_inventories"].shape[2]
    pol = orc.init_policy(policy, setting["problem_params"], F, 4321, setting["store_params"])
    res, _, grads = orc.train_step_gradients(pol, T, setting["problem_params"], data, obs)
    pol64 = orc.OraclePolicy(pol.name, [(w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True))
                                        for w, b in pol.layers], pol.inner_activation, pol.output_activation,
                             pol.warehouse_upper_bound.double(), pol.adjacency, pol.transshipment)
    _, _, g64 = orc.train_step_gradients(pol64, T, setting["problem_params"], {k: v.double() for k, v in data.items()}, obs)

    class _Sc:
        problem_params = setting["problem_params"]
        store_params = setting["store_params"]
    model = NeuralNetworkCreator().create_neural_network(_Sc(), policy, device=DEV)
    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(F)
    with torch.no_grad():
        for m, (w, b) in zip(model.master_linears(), pol.layers):
            m.weight.copy_(w.detach())
            m.bias.copy_(b.detach())
    model.warehouse_upper_bound = pol.warehouse_upper_bound.to(DEV)
    total, _ = eng.run({k: v.to(DEV) for k, v in data.items()}, T, 0, train=True, observation_params=obs)
    torch.cuda.synchronize()
    assert eng.dZhist is not None  # the all-period weight-gradient route
    assert abs(float(total) - float(res.total)) <= 1e-5 * abs(float(res.total))
    per_scn = eng.per_period_rewards().sum(dim=0).cpu()
    ref_scn = res.per_period.sum(dim=0)
    assert float(((per_scn - ref_scn).abs() / ref_scn.abs().clamp_min(1e-9)).max()) <= 1e-5
    for i, (p, ref32, ref64) in enumerate(zip(model.parameters(), grads, g64)):
        e_hip, e_ref = _rel(p.grad, ref64), _rel(ref32, ref64)
        print(f"tensor {i}: |HIP - fp64| = {e_hip:.2e}   |reference fp32 - fp64| = {e_ref:.2e}   |HIP - fp32| = {_rel(p.grad, ref32):.2e}")
        grad_parity_log.note_referee(i, e_hip, e_ref, _rel(p.grad, ref32), max(2.0 * e_ref, GRAD_TOL))
        assert e_hip <= max(2.0 * e_ref, GRAD_TOL), (i, e_hip, e_ref)  # (tensors already inside the 2e-5 bar need no referee)
        # ... and north_star's own bar against the reference's float32 gradient holds here too (recorded worst: 3.9e-6)
        assert _rel(p.grad, ref32) <= 1e-5, (i, _rel(p.grad, ref32))


@pytest.mark.parametrize("fused", [False, True])
def test_trainer_epochs_with_step_graph_match_eager_training(fused):
    """Three epochs of `Trainer.do_one_epoch` on a closed-form policy, eager vs `use_step_graph`: the same per-epoch losses
    and the same parameters after Adam.  fused = False: generic route (Simulator.step + autograd).  fused = True (the
    Trainer's default): the closed-form whole-horizon kernel inside the captured step - what `main_run`'s
    `use_step_graph: true` reaches through the PUBLIC epoch loop (several batches per epoch, a ragged last batch)."""
    from neural_inventory_control_amd.environment import Simulator
    from neural_inventory_control_amd.loss_functions import PolicyLoss
    from neural_inventory_control_amd.trainer import Trainer
    g = Golden("cfg2_one_store_backlogged_base_stock")
    c = g.fresh_config()
    ds = MyDataset(c["n"], {k: v.clone() for k, v in g.data.items()})

    def train(graph):
        torch.manual_seed(0)
        model = _model(g, c)
        sim = Simulator(device=DEV)
        with torch.no_grad():
            obs0, _ = sim.reset(c["periods"], c["problem_params"], {k: v.to(DEV) for k, v in g.data.items()},
                                c["observation_params"])
            o = dict(obs0)
            o["internal_data"] = sim._internal_data
            model(o)
        _load(model, g)
        opt = torch.optim.Adam(model.parameters(), lr=0.05)
        tr = Trainer(device=DEV)
        tr.use_fused_rollout = fused
        tr.use_step_graph = graph
        loader = DeviceBatches(ds, 20 if not fused else 16, shuffle=False, device=DEV)  # (16: a ragged last batch of 8)
        losses = [tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"],
                                  c["observation_params"], train=True, ignore_periods=c["ignore"])[1] for _ in range(3)]
        return losses, [p.detach().clone() for p in model.parameters()]

    (le, pe), (lg, pg) = train(False), train(True)
    if fused:
        assert c["n"] % 16  # the epoch really ends on a smaller batch (its own captured shape)
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * abs(a)
    for a, b in zip(pe, pg):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    assert le[-1] < le[0]  # and it learns


WAREHOUSE_CASES = [n for n in MLP_CASES if n.startswith(("cfg3", "cfg5", "x_transshipment"))]


@pytest.mark.parametrize("name", WAREHOUSE_CASES)
def test_fused_head_env_launches_equal_the_separate_ones(name):
    """Round 4 (csrc/head_env.hip): vanilla_warehouse head + env step in one launch, and env adjoint + head adjoint in one launch,
    are the same NIC_HD bodies run back to back - rewards, orders, states, logit gradients and parameter gradients are
    BIT-IDENTICAL to the three / four separate launches (one and several warehouses, 64 stores, transshipment)."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    out = {}
    for fuse in (True, False):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.fuse_head_env = fuse
        eng.fuse_tail = False   # (round 5: these shapes would otherwise take the fused tail launches, tested further down)
        eng.materialize(eng.input_rows(data, c["observation_params"]))
        _load(model, g)
        from neural_inventory_control_amd.rollout import KernelTimer
        eng.timer = KernelTimer(record_order=True)
        total, rep = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
        torch.cuda.synchronize()
        tags = {t for t, _ in eng.timer.order}
        assert ("head_env_fwd" in tags and "head_env_bwd" in tags and "env_fwd" not in tags and "head_bwd" not in tags) == fuse, tags
        out[fuse] = (float(total), float(rep), eng.per_period_rewards().clone(), eng.states.clone(), eng.orders.clone(),
                     [p.grad.clone() for p in model.parameters()])
    a, b = out[True], out[False]
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:5], b[2:5]):
        assert torch.equal(x, y)
    for x, y in zip(a[5], b[5]):
        assert torch.equal(x, y)
    _check_grads(model, g, GRAD_TOL)


@pytest.mark.parametrize("name", slim_case_names())
@pytest.mark.parametrize("rollout_graph", ["auto", False, True])
def test_trainer_at_the_shipped_batch_size_matches_reference(name, rollout_graph):
    """Round 4: the reference's shipped training batch - 1,024 scenarios x 50 periods, ignore 30
    (one_warehouse_lost_demand.yml:31-34) - through `Trainer.do_one_epoch`, on whatever route and launch mode the Trainer picks:
    per-scenario cost, totals and reported losses <= 1e-5, d(mean_loss)/d(theta) <= 1e-5 per parameter tensor, against numbers the
    REFERENCE produced at this batch size.  The inputs are rebuilt from the fixture's seeds by this package's `Scenario`
    (checksums of the reference's own tensors pinned).  Runs the epoch three times (eager, measured / captured, replayed)."""
    g = Golden(name)
    c = g.fresh_config()
    sc = Scenario(c["periods"], c["problem_params"], c["store_params"], c["warehouse_params"], c["echelon_params"], c["n"],
                  c["observation_params"], c["seeds"])
    data = sc.get_data()
    check_slim_inputs(g, data)
    model = _model(g, c, scenario=sc)
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    tr.use_rollout_graph = rollout_graph
    dev_data = {k: v.to(DEV) for k, v in data.items()}
    with torch.no_grad():   # materialise the lazy layers, then the fixture's weights
        obs0, _ = sim.reset(c["periods"], c["problem_params"], dev_data, c["observation_params"])
        o = dict(obs0)
        o["internal_data"] = sim._internal_data
        model(o)
    _load(model, g)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)   # (the step must not move the weights between the three epochs)
    loader = DeviceBatches(MyDataset(c["n"], data), c["n"], shuffle=False, device=DEV)
    S, T, ig = c["problem_params"]["n_stores"], c["periods"], c["ignore"]
    for rep in range(3):
        loss, report = tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, T, c["problem_params"], c["observation_params"],
                                       train=True, ignore_periods=ig)
        eng = tr._engines[(id(model), True)]
        assert type(eng).__name__ == "FusedRollout" and eng.small is None
        assert abs(loss - float(g.z["total"]) / (c["n"] * T * S)) <= 1e-5 * abs(loss)
        assert abs(report - float(g.z["reported"]) / (c["n"] * (T - ig) * S)) <= 1e-5 * abs(report)
        rewards, ref_r = eng.per_period_rewards().cpu(), g.tensor("rewards")
        tot_b, ref_b = rewards.double().sum(dim=0), ref_r.double().sum(dim=0)
        assert float(((tot_b - ref_b).abs() / ref_b.abs().clamp_min(1e-9)).max()) <= 1e-5
        _check_grads(model, g, GRAD_TOL)
    if rollout_graph is True:
        assert set(eng._graphs) == {"fwd", "bwd"}
    if rollout_graph == "auto":
        assert eng.auto_graph_probe is not None and eng.auto_graph_probe["replay"] == eng._graph_on()
    final = eng.final_state()
    for k, v in g.states(1).items():
        torch.testing.assert_close(final[k].cpu(), v, **STATE_TOL)
    # the small-batch route of round 4: weight gradients of the 256-wide layers contracted over (period group x scenario chunk)
    assert max(eng.splits) > c["n"] // 128


def test_step_graph_survives_dev_passes_of_another_horizon_at_the_same_batch_size():
    """with `use_step_graph` the captured closed-form training step replays into its engine's buffers by raw
    address; a dev pass with the SAME batch size but another horizon (the reference's configs: train 50 periods, dev 100) used
    to share that engine and re-size - free - those buffers.  Train and dev passes are interleaved here; the captured run must
    reproduce the eager run's losses and parameters (every (batch size, horizon, train / eval) context keeps its own engine)."""
    from neural_inventory_control_amd.environment import Simulator
    from neural_inventory_control_amd.loss_functions import PolicyLoss
    from neural_inventory_control_amd.trainer import Trainer
    g = Golden("cfg2_one_store_backlogged_base_stock")
    c = g.fresh_config()
    ds = MyDataset(c["n"], {k: v.clone() for k, v in g.data.items()})
    assert c["periods"] > 6

    def run(graph):
        torch.manual_seed(0)
        model = _model(g, c)
        sim = Simulator(device=DEV)
        with torch.no_grad():
            obs0, _ = sim.reset(c["periods"], c["problem_params"], {k: v.to(DEV) for k, v in g.data.items()},
                                c["observation_params"])
            o = dict(obs0)
            o["internal_data"] = sim._internal_data
            model(o)
        _load(model, g)
        opt = torch.optim.Adam(model.parameters(), lr=0.05)
        tr = Trainer(device=DEV)
        tr.use_step_graph = graph
        loader = DeviceBatches(ds, c["n"], shuffle=False, device=DEV)   # one batch per pass: train and dev share the batch size
        out = []
        for _ in range(4):
            out.append(tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"] - 5, c["problem_params"],
                                       c["observation_params"], train=True, ignore_periods=0)[0])
            # garbage the allocator can hand freed engine buffers to (what the saved best-params copy is in a real run)
            junk = [torch.full((c["n"] * 64,), float("nan"), device=DEV) for _ in range(8)]
            out.append(tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"],
                                       c["observation_params"], train=False, ignore_periods=2)[1])
            del junk
        return out, [p.detach().clone() for p in model.parameters()]

    (le, pe), (lg, pg) = run(False), run(True)
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * abs(a), (le, lg)
    for a, b in zip(pe, pg):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", QUANTILE_TRAINABLE)
def test_tape_route_training_step_replayed_from_a_graph_equals_eager_epochs(name):
    """The trainable quantile policies on the tape route are launch-bound (two whole-horizon launches inside ~40 small torch
    launches): `Trainer.use_step_graph = "auto"` captures their whole training step.  Four training epochs interleaved with dev
    passes of another horizon at the same batch size (and allocator churn in between), through `Trainer.do_one_epoch`: losses and
    parameters equal the eager run's; the training steps were replayed, the dev passes took the tape engine eagerly."""
    import time
    g = Golden(name)
    c = g.fresh_config()
    ds = MyDataset(c["n"], {k: v.clone() for k, v in g.data.items()})

    def run(graph):
        torch.manual_seed(0)
        model = _model(g, c)
        sim = Simulator(device=DEV)
        with torch.no_grad():
            obs0, _ = sim.reset(c["periods"], c["problem_params"], {k: v.to(DEV) for k, v in g.data.items()},
                                c["observation_params"])
            o = dict(obs0)
            o["internal_data"] = sim._internal_data
            model(o)
        _load(model, g)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        tr = Trainer(device=DEV)
        tr.use_step_graph = graph
        loader = DeviceBatches(ds, c["n"], shuffle=False, device=DEV)
        out, t_train = [], 0.0
        for ep in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out.append(tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"] - 3, c["problem_params"],
                                       c["observation_params"], train=True, ignore_periods=2)[0])
            torch.cuda.synchronize()
            if ep >= 3:
                t_train += time.perf_counter() - t0
            junk = [torch.full((c["n"] * 64,), float("nan"), device=DEV) for _ in range(8)]
            out.append(tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"],
                                       c["observation_params"], train=False, ignore_periods=2)[1])
            del junk
        assert any(type(e).__name__ == "TapeRollout" for e in tr._engines.values())
        assert bool(tr._step_graphs) == (graph in ("auto", True))
        return out, [p.detach().clone() for p in model.parameters()], t_train / 3

    (le, pe, te), (lg, pg, tg_) = run(False), run("auto")
    print(f"{name}: training epoch {te * 1e3:.2f} ms eager, {tg_ * 1e3:.2f} ms replayed")
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-6 * abs(a), (le, lg)
    for a, b in zip(pe, pg):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    assert le[0] != le[2]   # (the optimizer moved the policy)


def test_step_graph_refuses_capture_while_an_earlier_autograd_graph_is_alive():
    """A `total` returned by an eager `simulate_batch` and still held by the caller keeps the policy's gradient accumulators bound
    to the default stream; the autograd engine then synchronises the capture stream with it, which invalidates a capture (on this
    stack the process died in hipStreamEndCapture).  `_graphed_generic_step` notices during its side-stream warm-up, warns, and
    keeps eager steps for that batch shape: same losses as a trainer without step graphs; once the tensor is released a fresh
    trainer captures again."""
    import warnings
    g = Golden("f4_real_one_store_fixed_quantile")
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    ds = MyDataset(c["n"], {k: v.clone() for k, v in g.data.items()})
    loader = DeviceBatches(ds, c["n"], shuffle=False, device=DEV)

    def fresh():
        torch.manual_seed(0)
        model = _model(g, g.fresh_config())
        sim = Simulator(device=DEV)
        with torch.no_grad():
            o = dict(sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])[0])
            o["internal_data"] = sim._internal_data
            model(o)
        _load(model, g)
        return model, sim, torch.optim.Adam(model.parameters(), lr=1e-3)

    def epochs(tr, model, sim, opt, n=4):
        return [tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, c["periods"], c["problem_params"], c["observation_params"],
                                train=True, ignore_periods=c["ignore"])[0] for _ in range(n)]

    model, sim, opt = fresh()
    tr0 = Trainer(device=DEV)
    held, _ = tr0.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data, c["observation_params"],
                                 c["ignore"], False)     # an eager result the caller keeps (its autograd graph stays alive)
    assert held.requires_grad
    tr = Trainer(device=DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = epochs(tr, model, sim, opt)
    assert any("not captured into a HIP graph" in str(w.message) for w in caught)
    assert all(st.get("eager_only") for st in tr._step_graphs.values())
    model2, sim2, opt2 = fresh()
    tr2 = Trainer(device=DEV)
    tr2.use_step_graph = False
    want = epochs(tr2, model2, sim2, opt2)
    for a, b in zip(got, want):
        assert abs(a - b) <= 2e-6 * abs(b), (got, want)
    del held
    model3, sim3, opt3 = fresh()
    tr3 = Trainer(device=DEV)
    again = epochs(tr3, model3, sim3, opt3)
    assert any("graph" in st for st in tr3._step_graphs.values())      # captured this time
    for a, b in zip(again, want):
        assert abs(a - b) <= 2e-6 * abs(b), (again, want)


# ---- closed-form policies: whole horizon + forward-mode gradient in one kernel (csrc/closed_form.hip) -------------------

CLOSED_FORM_CASES = ["cfg2_one_store_backlogged_base_stock", "cfg2_one_store_backlogged_capped", "cfg4_serial_echelon_stock"]


@pytest.mark.parametrize("name", CLOSED_FORM_CASES)
def test_closed_form_kernel_matches_reference(name):
    """nic_closed_form_rollout through the C ABI against the reference's golden vectors (rewards, final state, gradient)."""
    import closed_form_checks as cfc
    worst = cfc.check_against_golden(cfc.run_case(name, cfc.hip_launch(), DEV))
    assert worst <= GRAD_TOL


@pytest.mark.parametrize("seed", range(12))
def test_closed_form_chain_on_random_serial_systems_matches_oracle(seed):
    """1-3 extra echelons, random lead times / costs / demand moments / lost-demand and profit switches, n and T off the
    kernel's batch sizes: the chain kernel through the C ABI against the oracle's autograd (per-period costs, gradient of the
    mean cost with respect to the policy's parameters at 1e-5)."""
    import closed_form_checks as cfc
    assert cfc.check_random_serial_case(seed, cfc.hip_launch(), DEV) <= GRAD_TOL


@pytest.mark.parametrize("name", CLOSED_FORM_CASES)
def test_trainer_takes_closed_form_route_and_matches_reference(name):
    """`Trainer.simulate_batch` + the reference idiom `(total / n).backward()` on a closed-form policy: one kernel for the
    horizon, gradients reach net.master.0.* through autograd; same numbers as the generic Simulator.step route."""
    from neural_inventory_control_amd.closed_form import ClosedFormRollout
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    n = c["n"] * c["periods"] * c["problem_params"]["n_stores"]
    res = {}
    for fused in (True, False):
        model = _model(g, c)
        sim, tr = Simulator(device=DEV), Trainer(device=DEV)
        tr.use_fused_rollout = fused
        with torch.no_grad():
            obs, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
            o = dict(obs)
            o["internal_data"] = sim._internal_data
            model(o)  # materialises the lazy layer
        _load(model, g)
        model.zero_grad()
        total, reported = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data,
                                            c["observation_params"], c["ignore"], False)
        (total / n).backward()
        torch.cuda.synchronize()
        took = any(isinstance(e, ClosedFormRollout) for e in tr._engines.values())
        assert took == fused
        assert abs(float(total) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))
        assert abs(float(reported) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
        _check_grads(model, g, GRAD_TOL)
        res[fused] = float(total)
        # evaluation (no_grad) and discrete allocation run the same kernel without tangents
        with torch.no_grad():
            t_eval, _ = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data,
                                          c["observation_params"], c["ignore"], False)
            t_disc, _ = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data,
                                          c["observation_params"], c["ignore"], True)
        assert abs(float(t_eval) - float(total)) <= 1e-6 * abs(float(total))
        res[(fused, "disc")] = float(t_disc)
    assert abs(res[True] - res[False]) <= 2e-6 * abs(res[False])
    assert abs(res[(True, "disc")] - res[(False, "disc")]) <= 2e-6 * abs(res[(False, "disc")])
    assert res[(True, "disc")] != res[True]


@pytest.mark.parametrize("policy_name", ["base_stock", "capped_base_stock"])
@pytest.mark.parametrize("Ws", [2, 3, 4])
def test_closed_form_specialised_variants_equal_the_generic_kernel(policy_name, Ws):
    """Round 5: single-store chains whose lead-time table does not vary over the scenarios run `closed_form_kernel<NP,4,false,Ws>`
    (pipeline length compiled in, the order placed by one wave-uniform branch, lost-demand / profit / rounding resolved in front
    of the period loop).  Same arithmetic in the same order as the generic kernel: rewards, totals, final state and the level
    gradients are BIT-IDENTICAL, for every combination of the three switches, pipeline lengths 2-4, lead times 1..Ws, with and
    without tangents, on a batch that does not fill its last wavefront.  (The generic kernel is reached by handing the same
    lead times over as a per-scenario table.)"""
    from neural_inventory_control_amd import closed_form as cf, _lib as L
    from neural_inventory_control_amd.layout import EnvProblem
    B, S, T = 300, 3, 13
    gen = torch.Generator().manual_seed(Ws * 7 + len(policy_name))
    for lost in (True, False):
        for profit in (True, False):
            for rounded in (False, True):
                pp = {"n_stores": S, "n_warehouses": 0, "n_extra_echelons": 0, "lost_demand": lost, "maximize_profit": profit}
                lead = torch.randint(1, Ws + 1, (S,), generator=gen).float()
                data = {"demands": (torch.rand(B, S, T, generator=gen) * 8).to(DEV),
                        "initial_inventories": (torch.rand(B, S, Ws, generator=gen) * 6).to(DEV),
                        "underage_costs": torch.full((B, S), 9.0, device=DEV), "holding_costs": torch.full((B, S), 1.0, device=DEV),
                        "lead_times": lead.to(DEV).expand(B, S).contiguous()}
                prob = EnvProblem(pp, data, DEV)
                assert prob.lead.scn_stride == 0 and prob.Ws == Ws
                ld = prob.ldb
                levels = torch.tensor([11.5, 7.25][:1 if policy_name == "base_stock" else 2], device=DEV)
                demand = torch.zeros(T, S, ld, device=DEV)
                demand[:, :, :B] = data["demands"].permute(2, 1, 0)
                state0 = cf.pack_state0(data, prob)
                per_scn = torch.zeros(S, ld, device=DEV)
                per_scn[:, :B] = lead.to(DEV)[:, None]
                res = {}
                for which in ("specialised", "generic"):
                    desc = cf.make_desc(prob, policy_name, T, 0, 4, levels, demand, state0, round_orders=rounded)
                    if which == "generic":
                        desc.lead = L.NicTable2(per_scn.data_ptr(), ld, 1)
                    outs = []
                    for want_grad in ([False] if rounded else [True, False]):
                        rewards, totals, final = torch.zeros(T, S, ld, device=DEV), torch.zeros(2, S, ld, device=DEV), \
                            torch.zeros(S, Ws, ld, device=DEV)
                        n_part = L.lib().nic_closed_form_num_partials(B, S)
                        part = torch.zeros(n_part, levels.numel() + 2, device=DEV)
                        L.check(L.lib().nic_closed_form_rollout_sums(desc, rewards.data_ptr(), totals.data_ptr(), final.data_ptr(),
                                                                     part.data_ptr(), levels.numel() + 2, int(want_grad), 1,
                                                                     L.current_stream()))
                        torch.cuda.synchronize()
                        name = (L.lib().nic_last_kernel() or b"").decode()
                        assert name.endswith(f",false,{Ws}>") == (which == "specialised"), name
                        ng = levels.numel() if want_grad else 0
                        # the per-wavefront sums add up to the per-chain totals
                        assert abs(float(part[:, ng].double().sum()) - float(totals[0].double().sum())) <= 1e-6 * abs(float(totals[0].double().sum()))
                        outs.append((rewards, totals, final, part))
                    res[which] = outs
                for a, b in zip(res["specialised"], res["generic"]):
                    for x, y in zip(a, b):
                        assert torch.equal(x, y), (lost, profit, rounded)


def test_closed_form_multi_store_and_training():
    """base_stock on 5 independent stores (Wn = 0): every store is its own chain (grid.y); a few Adam steps through
    `Trainer.do_one_epoch` lower the cost, and the fused route follows the generic route step for step."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    setting, policy, _, _, _ = workloads.get("base_stock")
    setting["problem_params"]["n_stores"] = 5
    setting["store_params"]["demand"].update(mean=[5.0, 3.0, 6.0, 4.0, 7.0], std=[1.6, 1.0, 2.0, 1.2, 2.5], correlation=0.3)
    setting["store_params"]["lead_time"] = {"sample_across_stores": True, "vary_across_samples": False, "expand": False,
                                            "range": [2, 5]}
    obs = defaultdict(lambda: None, setting["observation_params"])
    T, n = 40, 300
    finals = {}
    for fused in (True, False):
        import copy
        sc = Scenario(T, setting["problem_params"], copy.deepcopy(setting["store_params"]), None, None, n, obs,
                      dict(setting["seeds"]))
        ds = DatasetCreator().create_datasets(sc, split=False)
        torch.manual_seed(3)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        opt = torch.optim.Adam(model.parameters(), lr=0.3)
        tr, sim = Trainer(device=DEV), Simulator(device=DEV)
        tr.use_fused_rollout = fused
        loader = DeviceBatches(ds, 128, shuffle=False, device=DEV)
        losses = [tr.do_one_epoch(opt, loader, PolicyLoss(), sim, model, T, setting["problem_params"], obs, train=True,
                                  ignore_periods=10)[1] for _ in range(6)]
        assert losses[-1] < losses[0]
        finals[fused] = (losses, [p.detach().clone() for p in model.parameters()])
    for a, b in zip(finals[True][0], finals[False][0]):
        assert abs(a - b) <= 1e-5 * abs(b)
    for a, b in zip(finals[True][1], finals[False][1]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


# ---- GNN policy: fused gather-MLP kernels over the static supply graph (gnn_rollout.py, csrc/mlp3.hip) --------------------

GNN_CASES = ["f1_one_warehouse_gnn", "f1_one_warehouse_16_gnn", "f1_one_warehouse_gnn_transshipment",
             "f1_many_warehouses_2x10_gnn", "f1_many_warehouses_3x8_dense_gnn"]


@pytest.mark.parametrize("fused_bwd", [True, "hist", "hist_stored_inputs", "period"])
@pytest.mark.parametrize("name", GNN_CASES)
def test_gnn_fused_rollout_matches_reference(name, fused_bwd):
    """`GnnRollout` (five fused gather-MLP launches per period, segment-sum aggregation, manual backward sweep) against the
    reference's golden vectors: per-period rewards, per-scenario cost, final state and d(mean_loss)/d(theta) of all 30 tensors."""
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    g = Golden(name)
    c = g.fresh_config()
    model = _model(g, c)
    assert GnnRollout.supports(model, c["problem_params"])
    eng = GnnRollout(model, c["problem_params"], DEV)
    # history-free backward with in-kernel weight gradients / stored activations + GEMMs / stored activations with in-kernel
    # weight gradients, with and without the stored copy of the gathered inputs
    # ... "period": the whole backward of a period in one launch (csrc/gnn_period_bwd.hip, round 6) - "hist" keeps the per-MLP launches
    eng.fused_bwd = "hist" if fused_bwd in ("hist_stored_inputs", "period") else fused_bwd
    eng.keep_inputs = fused_bwd == "hist_stored_inputs"
    eng.use_period_bwd = fused_bwd == "period"
    data = {k: v.to(DEV) for k, v in g.data.items()}
    Dn = max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4
    eng.materialize(Dn)
    _load(model, g)
    total, reported = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
    torch.cuda.synchronize()
    assert eng._period_bwd == (fused_bwd == "period")
    rewards = eng.per_period_rewards().cpu()
    want = _Expected(g, c)
    ref_r = want.rewards
    torch.testing.assert_close(rewards, ref_r, rtol=1e-5, atol=1e-4)
    tot_b, ref_b = rewards.double().sum(dim=0), ref_r.double().sum(dim=0)
    assert float(((tot_b - ref_b).abs() / ref_b.abs().clamp_min(1e-9)).max()) <= 1e-5
    assert abs(float(total) - want.total) <= 1e-5 * abs(want.total)
    assert abs(float(reported) - want.reported) <= 1e-5 * abs(want.reported)
    final = eng.final_state()
    for k, v in want.final.items():
        torch.testing.assert_close(final[k].cpu(), v, **STATE_TOL)
    ref = want.grads
    named = dict(model.named_parameters())
    worst = 0.0
    for k, r in ref.items():
        rel = float((named[k].grad.cpu() - r).norm() / (r.norm() + 1e-30))
        worst = max(worst, rel)
        assert rel <= GRAD_TOL, (k, rel)
    print(f"{name}: worst relative gradient error {worst:.2e}")
    # evaluation mode gives the same costs; the Trainer takes this route by itself
    t2, _ = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
    assert abs(float(t2) - float(total)) <= 1e-6 * abs(float(total))
    tr = Trainer(device=DEV)
    model.zero_grad()
    tot3, _ = tr.simulate_batch(PolicyLoss(), Simulator(device=DEV), model, c["periods"], c["problem_params"], data,
                                c["observation_params"], c["ignore"], False)
    assert any(isinstance(e, GnnRollout) for e in tr._engines.values())
    (tot3 / (c["n"] * c["periods"] * c["problem_params"]["n_stores"])).backward()
    for k, r in ref.items():
        assert float((named[k].grad.cpu() - r).norm() / (r.norm() + 1e-30)) <= GRAD_TOL, k


@pytest.mark.parametrize("name", ["f1_one_warehouse_gnn", "f1_many_warehouses_3x8_dense_gnn"])
def test_gnn_graph_replay_matches_eager(name):
    """The GNN engine's launch sequence (fused MLP launches, segment sums, the small allocation ops, env steps, the batched
    weight gradients) captured into HIP graphs and replayed: same costs and gradients as eager launches, also after the batch
    contents change."""
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    data2 = dict(data)
    data2["demands"] = (data["demands"] * 1.3 + 0.25).contiguous()
    out = {}
    for mode in ("eager", "graph", "auto"):
        model = _model(g, c)
        eng = GnnRollout(model, c["problem_params"], DEV)
        eng.use_graph = {"eager": False, "graph": True, "auto": "auto"}[mode]
        eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
        _load(model, g)
        res = []
        for d in (data, data2, data, data2, data, data2):
            total, rep = eng.run(d, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
            torch.cuda.synchronize()
            res.append((float(total), float(rep), [p.grad.clone() for p in model.parameters()]))
        out[mode] = res
        if mode == "graph":
            assert len(eng._graphs) == 2
        if mode == "auto":
            # round 4: decided by measurement on the second training run (what `Trainer` sets on its engines) - a fixture-sized
            # batch is launch-bound on any host, so the later runs were replayed
            # round 6: three launches per period - a fixture-sized step is no longer launch-bound on every host; what is checked is
            # the probe's rule: later runs are replayed if and only if it said so
            pr = eng.auto_graph_probe
            assert pr is not None and pr["replay"] == (pr["host_enqueue_ms"] > 0.85 * pr["gpu_ms"])
            assert len(eng._graphs) == (2 if pr["replay"] else 0)
    for mode in ("graph", "auto"):
        for a, b in zip(out["eager"], out[mode]):
            assert a[0] == b[0] and a[1] == b[1]
            for x, y in zip(a[2], b[2]):
                assert torch.equal(x, y)
    assert out["eager"][0][0] != out["eager"][1][0]
    # ... and `Trainer.simulate_batch` hands its own setting to the engine it creates
    tr = Trainer(device=DEV)
    model = _model(g, c)
    sim = Simulator(device=DEV)
    with torch.no_grad():
        o = dict(sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])[0])
        o["internal_data"] = sim._internal_data
        model(o)
    _load(model, g)
    if "mean" in data and "std" in data:
        tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data, c["observation_params"], c["ignore"],
                          False, train=True)
        engines = [e for e in tr._engines.values() if isinstance(e, GnnRollout)]
        assert engines and engines[0].use_graph == "auto"


@pytest.mark.parametrize("name", ["f1_one_warehouse_gnn", "f1_one_warehouse_16_gnn", "f1_one_warehouse_gnn_transshipment"])
def test_gnn_fused_alloc_env_launches_equal_the_separate_ones(name):
    """Round 4: on one-warehouse graphs the GNN engine runs the allocation head and the env step in ONE launch per direction
    (csrc/gnn_alloc_env.hip: the two bodies back to back with a workgroup barrier in between).  Same bodies, same order of
    operations: costs, per-period rewards, final state and every gradient are BIT-IDENTICAL to the separate launches."""
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    from neural_inventory_control_amd.rollout import KernelTimer
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    out = {}
    for fused in (True, False):
        model = _model(g, c)
        eng = GnnRollout(model, c["problem_params"], DEV)
        eng.fuse_alloc_env = fused
        eng.use_period_kernel = False   # (the period kernel carries the allocation + env step itself; this is about the two launches)
        eng.use_period_bwd = False      # (... and so does the period backward kernel, round 6)
        eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
        _load(model, g)
        eng.timer = KernelTimer(record_order=True)
        total, rep = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
        torch.cuda.synchronize()
        tags = {t for t, _ in eng.timer.order}
        assert ("alloc_env_fwd" in tags and "alloc_env_bwd" in tags and "env_fwd" not in tags) == fused
        out[fused] = (float(total), float(rep), eng.rewards.clone(), eng.states[-1].clone(), [p.grad.clone() for p in model.parameters()])
    a, b = out[True], out[False]
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for x, y in zip(a[4], b[4]):
        assert torch.equal(x, y)
    assert abs(a[0] - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))


@pytest.mark.parametrize("n", [1000, 8192 + 5])
def test_gnn_period_kernel_at_ragged_batch_sizes(n):
    """The period kernel's 16-scenario blocks at batch sizes that are not a multiple of 16 (a half-filled last block: its dead
    lanes compute on zeros and must store nothing) and not a multiple of 32 (half a native history block per entity): costs,
    per-period rewards, final state and every gradient against the per-MLP launches on the bench's GNN workload; the padding
    columns of the state stay zero."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    setting, policy, _, _, _ = workloads.get("gnn")
    obs = defaultdict(lambda: None, setting["observation_params"])
    T = 6
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, dict(setting["seeds"]), sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    out = {}
    for period in (True, False):
        torch.manual_seed(3)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng = GnnRollout(model, setting["problem_params"], DEV)
        eng.use_period_kernel = period
        eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
        total, rep = eng.run(data, T, 2, train=True, observation_params=setting["observation_params"], demand_soa=sc.demands_soa)
        torch.cuda.synchronize()
        assert eng._period == period
        assert float(eng.states[:, :, n:].abs().max()) == 0.0 if eng.states.shape[2] > n else True
        out[period] = (float(total), float(rep), eng.rewards[:, :n].clone(), eng.states[-1][:, :n].clone(),
                       [p.grad.clone() for p in model.parameters()])
    a, b = out[True], out[False]
    assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-6 * abs(b[1])
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(a[3], b[3], rtol=1e-5, atol=1e-4)
    for x, y in zip(a[4], b[4]):
        assert float((x - y).norm() / (y.norm() + 1e-30)) <= 1e-5


@pytest.mark.parametrize("slots,variant", [(7, "gnn_period_fwd_kernel<8,"), (11, "gnn_period_fwd_kernel<16,")])
def test_gnn_period_kernel_with_long_pipelines(slots, variant):
    """The period kernel's variants for store pipelines of more than 4 slots (env bodies instantiated for 8 / 16 slots, eight
    wavefronts per workgroup instead of sixteen) - no golden fixture has such pipelines on a one-warehouse graph: training and
    evaluation runs against the per-MLP launches + `nic_gnn_alloc_env_fwd` on a 5-store setting with lead times up to `slots`."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    from neural_inventory_control_amd.rollout import KernelTimer
    setting, policy, _, _, _ = workloads.get("gnn")
    setting["problem_params"]["n_stores"] = 5
    setting["store_params"]["lead_time"] = {"sample_across_stores": True, "vary_across_samples": False, "expand": False,
                                            "range": [2, slots + 1]}
    setting["store_params"]["initial_inventory"]["inventory_periods"] = slots
    obs = defaultdict(lambda: None, setting["observation_params"])
    T, n = 2 * slots, 200
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, dict(setting["seeds"]), sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    assert data["initial_inventories"].shape[2] == slots and int(data["lead_times"].max()) > 4
    for train in (True, False):
        out = {}
        for period in (True, False):
            torch.manual_seed(3)
            model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
            eng = GnnRollout(model, setting["problem_params"], DEV)
            eng.use_period_kernel = period
            eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
            eng.timer = KernelTimer(record_order=True)
            total, rep = eng.run(data, T, 3, train=train, observation_params=setting["observation_params"], demand_soa=sc.demands_soa)
            torch.cuda.synchronize()
            if period:
                assert any(k.startswith(variant) for _, k in eng.timer.order), sorted({k for _, k in eng.timer.order})
            out[period] = (float(total), float(rep), eng.rewards[:, :n].clone(), eng.states[-1][:, :n].clone(),
                           [p.grad.clone() for p in model.parameters()] if train else [])
        a, b = out[True], out[False]
        assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-6 * abs(b[1])
        torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(a[3], b[3], rtol=1e-5, atol=1e-4)
        for x, y in zip(a[4], b[4]):
            assert float((x - y).norm() / (y.norm() + 1e-30)) <= 1e-5


def test_gnn_period_kernel_differential_fuzz():
    """The period kernel against the per-MLP launches on random one-warehouse settings the fixtures do not cover: 2-16 stores (16:
    the largest one-warehouse graph whose embeddings fit in LDS), store / warehouse pipelines of 2-9 / 2-5 slots, with and without transshipment,
    edge costs on and off, batches of 17-300 scenarios, training and evaluation."""
    import random
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    rng = random.Random(20260501)
    for trial in range(8):
        S = rng.choice([2, 3, 5, 9, 12, 14, 16])
        Ws, wlead = rng.randint(2, 9), rng.randint(2, 5)
        setting, policy, _, _, _ = workloads.get("gnn")
        setting["problem_params"]["n_stores"] = S
        setting["store_params"]["lead_time"] = {"sample_across_stores": True, "vary_across_samples": False, "expand": False,
                                                "range": [1, Ws + 1]}
        setting["store_params"]["initial_inventory"]["inventory_periods"] = Ws
        setting["warehouse_params"]["lead_time"] = wlead
        if rng.random() < 0.5:
            setting["warehouse_params"]["edge_cost"] = 0.7
        policy["transshipment"] = rng.random() < 0.4
        obs = defaultdict(lambda: None, setting["observation_params"])
        n, T = rng.randint(17, 300), rng.randint(3, 6)
        sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                      n, obs, dict(setting["seeds"]), sampler="hip", device=DEV)
        data = {k: v.to(DEV) for k, v in sc.get_data().items()}
        train = trial % 3 != 2
        out = {}
        for period in (True, False):
            torch.manual_seed(trial)
            model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
            if not GnnRollout.supports(model, setting["problem_params"]):
                break
            eng = GnnRollout(model, setting["problem_params"], DEV)
            eng.use_period_kernel = period
            eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
            total, rep = eng.run(data, T, 1, train=train, observation_params=setting["observation_params"], demand_soa=sc.demands_soa)
            torch.cuda.synchronize()
            assert eng._period == period, (S, Ws, wlead)
            out[period] = (float(total), float(rep), eng.rewards[:, :n].clone(), eng.states[-1][:, :n].clone(),
                           [p.grad.clone() for p in model.parameters()] if train else [])
        if len(out) < 2:
            continue
        a, b = out[True], out[False]
        tag = dict(trial=trial, S=S, Ws=Ws, wlead=wlead, n=n, T=T, train=train, trans=policy["transshipment"])
        assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2e-6 * abs(b[1]), tag
        torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(a[3], b[3], rtol=1e-5, atol=1e-4)
        for x, y in zip(a[4], b[4]):   # (+ an absolute floor: a horizon shorter than the lead times leaves gradients of ~1e-11)
            assert float((x - y).norm()) <= 1e-5 * float(y.norm()) + 1e-9, tag


def test_initial_inventories_written_behind_torchs_back_are_seen():
    """A batch tensor rewritten WITHOUT a version bump (`.data` copy - what a raw-pointer kernel or `set_()` also looks like to
    torch) must still reach the whole-horizon kernels: by default every presented batch is copied into the engine's state
    block; only `inputs_versioned = True` (bench.py) may skip the copy of an 'unchanged' tensor - and then does miss it."""
    g = Golden("cfg2_one_store_backlogged_vanilla")
    c = g.fresh_config()
    data = {k: v.to(DEV).clone() for k, v in g.data.items()}
    out = {}
    for versioned in (False, True):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.inputs_versioned = versioned
        eng.materialize(data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2])
        _load(model, g)
        inv = data["initial_inventories"]
        keep = inv.clone()
        t1, _ = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
        assert eng.small is not None   # (the route that keeps the state block)
        v0 = inv._version
        inv.data.copy_(keep + 3.0)   # no version bump
        assert inv._version == v0
        t2, _ = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
        out[versioned] = (float(t1), float(t2))
        inv.data.copy_(keep)
    assert out[False][0] == out[True][0]
    assert out[False][1] != out[False][0]        # default: the write is seen
    assert out[True][1] == out[True][0]          # opt-in skip: it is not (documented)


def test_simulator_upstream_zero_lead_mode_on_the_hand_computed_period_and_the_fixture():
    """`Simulator.zero_lead_orders = "upstream"`: (1) the hand-computed period of kernel_checks.zero_lead_micro_case - the order of 4
    on a column without a lead time lands on the LAST element of the batch (one scenario: store 1's last slot), everything else as
    in "drop" mode, and its gradient is the gradient of that element; (2) `Trainer.simulate_batch` on the reference's sparse
    many-warehouse GNN fixture reproduces the reference's own totals on BOTH routes (generic Simulator.step loop, fused engine) -
    the trainer hands the simulator's rule to the engine."""
    import kernel_checks as kc
    problem, data, action, want, obs_params = kc.zero_lead_micro_case()
    sim = Simulator(device=DEV)
    sim.zero_lead_orders = "upstream"
    sim.reset(1, problem, {k: v.to(DEV) for k, v in data.items()}, obs_params)
    a = {k: v.to(DEV).requires_grad_() for k, v in action.items()}
    obs, reward, _, _, _ = sim.step(a)
    leak = want["store_inventories"].clone()
    leak[0, 1, 2] += 4.0
    assert torch.equal(obs["store_inventories"].detach().cpu(), leak)
    assert torch.equal(obs["warehouse_inventories"].detach().cpu(), want["warehouse_inventories"])
    assert torch.equal(reward.detach().cpu(), want["reward"])
    obs["store_inventories"][0, 1, 2].backward()
    g_a = a["stores"].grad.cpu()
    assert float(g_a[0, 0, 0]) == 1.0 and float(g_a[0, 1, 0]) == 1.0   # the misplaced 4, and store 1's own order with lead time 3
    g = Golden("f1_many_warehouses_2x10_gnn")
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    for fused in (False, True):
        model = _model(g, c)
        sim, tr = Simulator(device=DEV), Trainer(device=DEV)
        sim.zero_lead_orders = "upstream"
        tr.use_fused_rollout = fused
        with torch.no_grad():
            obs0, _ = sim.reset(c["periods"], c["problem_params"], data, c["observation_params"])
            o = dict(obs0)
            o["internal_data"] = sim._internal_data
            model(o)
        _load(model, g)
        model.zero_grad()
        total, reported = tr.simulate_batch(PolicyLoss(), sim, model, c["periods"], c["problem_params"], data,
                                            c["observation_params"], c["ignore"], False)
        (total / (c["n"] * c["periods"] * c["problem_params"]["n_stores"])).backward()
        assert abs(float(total) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"])), fused
        assert abs(float(reported) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
        _check_grads(model, g, GRAD_TOL)


@pytest.mark.parametrize("period", [True, False])
def test_gnn_upstream_zero_lead_mode_matches_the_reference_itself(period):
    """`GnnRollout.zero_lead_orders = "upstream"`: on the sparse many-warehouse fixture - where the reference's GNN books some
    store orders on a column whose lead time is 0 and its env step then adds them to the element in front of the store's pipeline
    (previous store / previous scenario) - the engine reproduces the REFERENCE's own golden numbers (rewards, totals, final state,
    all 30 gradients), not the oracle's "drop" variant the default mode is compared with."""
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    g = Golden("f1_many_warehouses_2x10_gnn")
    c = g.fresh_config()
    model = _model(g, c)
    eng = GnnRollout(model, c["problem_params"], DEV)
    eng.zero_lead_orders = "upstream"
    eng.use_period_kernel = period
    data = {k: v.to(DEV) for k, v in g.data.items()}
    eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
    _load(model, g)
    total, reported = eng.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
    torch.cuda.synchronize()
    assert eng._zl_pairs   # the fixture does have such columns
    torch.testing.assert_close(eng.per_period_rewards().cpu(), g.tensor("rewards"), rtol=1e-5, atol=1e-4)
    assert abs(float(total) - float(g.z["total"])) <= 1e-5 * abs(float(g.z["total"]))
    assert abs(float(reported) - float(g.z["reported"])) <= 1e-5 * abs(float(g.z["reported"]))
    final = eng.final_state()
    for k, v in g.states(c["periods"]).items():
        torch.testing.assert_close(final[k].cpu(), v, **STATE_TOL)
    _check_grads(model, g, GRAD_TOL)


@pytest.mark.parametrize("mode", ["hist", True, "eval"])
@pytest.mark.parametrize("name", GNN_CASES)
def test_gnn_period_kernel_matches_the_per_mlp_launches(name, mode):
    """Round 5: ONE forward launch per period (csrc/gnn_period.hip: the five MLPs on node / edge embeddings held in LDS, then
    allocation + env step on one-warehouse graphs) against the per-MLP launches of csrc/mlp3.hip on the same weights and batch.
    Other MFMA shape, other accumulation order: equal to rounding (costs 1e-6, gradients 1e-5 per tensor), and the golden total."""
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    from neural_inventory_control_amd.rollout import KernelTimer
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    train = mode != "eval"
    out = {}
    for period in (True, False):
        model = _model(g, c)
        eng = GnnRollout(model, c["problem_params"], DEV)
        eng.use_period_kernel = period
        if train:
            eng.fused_bwd = mode
        eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
        _load(model, g)
        eng.timer = KernelTimer(record_order=True)
        total, rep = eng.run(data, c["periods"], c["ignore"], train=train, observation_params=c["observation_params"])
        torch.cuda.synchronize()
        tags = {t for t, _ in eng.timer.order}
        assert ("gnn_period_fwd" in tags) == period and ("mlp3_fwd_initial_node" in tags) != period
        if period and c["problem_params"]["n_warehouses"] == 1:
            assert "alloc_env_fwd" not in tags and "env_fwd" not in tags    # allocation + env step ran inside the launch
        out[period] = (float(total), float(rep), eng.rewards.clone(), eng.states[-1].clone(),
                       [p.grad.clone() for p in model.parameters()] if train else [])
    a, b = out[True], out[False]
    assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-6 * abs(b[1])
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(a[3], b[3], rtol=1e-5, atol=1e-4)
    for x, y in zip(a[4], b[4]):
        assert float((x - y).norm() / (y.norm() + 1e-30)) <= 1e-5
    want = _Expected(g, c).total
    assert abs(a[0] - want) <= 1e-5 * abs(want)


def _gnn_run_pair(setting, policy, n, T, seed, train=True, ignore=1, **switches):
    """One GNN training run per value of the switches' tuples (e.g. use_period_bwd=(True, False)) on the same data and weights."""
    from collections import defaultdict
    from neural_inventory_control_amd.gnn_rollout import GnnRollout
    from neural_inventory_control_amd.rollout import KernelTimer
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, dict(setting["seeds"]), sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    out = []
    for i in range(len(next(iter(switches.values())))):
        torch.manual_seed(seed)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        if not GnnRollout.supports(model, setting["problem_params"]):
            return None
        eng = GnnRollout(model, setting["problem_params"], DEV)
        for k, v in switches.items():
            setattr(eng, k, v[i])
        eng.materialize(max(data["initial_inventories"].shape[2], data["initial_warehouse_inventories"].shape[2]) + 4)
        eng.timer = KernelTimer(record_order=True)
        total, rep = eng.run(data, T, ignore, train=train, observation_params=setting["observation_params"], demand_soa=sc.demands_soa)
        torch.cuda.synchronize()
        out.append(dict(total=float(total), rep=float(rep), rewards=eng.rewards[:, :n].clone(), state=eng.states[-1][:, :n].clone(),
                        grads=[p.grad.clone() for p in model.parameters()] if train else [],
                        names=[k for k, _ in model.named_parameters()], tags={t for t, _ in eng.timer.order}, eng=eng))
    return out


def _assert_same_gradients(a, b, tol=1e-5, floor=1e-9, tag=None):
    assert a["total"] == b["total"] and a["rep"] == b["rep"], tag     # (same forward)
    for name, x, y in zip(a["names"], a["grads"], b["grads"]):
        assert float((x - y).norm()) <= tol * float(y.norm()) + floor, (tag, name, float((x - y).norm() / (y.norm() + 1e-30)))


@pytest.mark.parametrize("workload,n,T", [("gnn", 1000, 6), ("gnn", 8192 + 5, 3), ("gnn", 16400, 2), ("gnn_many_warehouses", 700, 5),
                                          ("gnn_many_warehouses", 8192, 2)])
def test_gnn_period_backward_matches_the_per_mlp_launches(workload, n, T):
    """Round 6: the backward of a period as ONE launch (csrc/gnn_period_bwd.hip: five MLP adjoints with in-kernel weight gradients,
    every adjoint gather as "sum the pre-activation gradients over a node's edges, multiply once", the aggregation's adjoint, the
    row adds into the state gradient) against round 5's five `nic_mlp3_bwd_hist` + three `nic_segment_sum_terms` launches on the
    bench's two GNN workloads: ragged batches (a half-filled last 16-scenario block, half a native history block), batches of one
    and two blocks per workgroup, more than one round of workgroups, and a graph (89 entities) that no LDS-resident design holds."""
    from neural_inventory_control_amd import workloads
    setting, policy, _, _, _ = workloads.get(workload)
    a, b = _gnn_run_pair(setting, policy, n, T, 3, use_period_bwd=(True, False))
    assert a["eng"]._period_bwd and not b["eng"]._period_bwd
    assert "gnn_period_bwd" in a["tags"] and not any(t.startswith("mlp3_bwd") for t in a["tags"])
    if workload == "gnn":   # one warehouse: the env / allocation adjoint runs inside the same launch
        assert "alloc_env_bwd" not in a["tags"] and "alloc_env_bwd" in b["tags"]
    assert "gnn_period_bwd" not in b["tags"] and "mlp3_bwd_edge_update" in b["tags"]
    _assert_same_gradients(a, b, tag=(workload, n, T))


@pytest.mark.parametrize("workload,stores,n,T,train", [("gnn_many_warehouses", 16, 700, 4, True), ("gnn_many_warehouses", 16, 8192 + 5, 2, True),
                                                       ("gnn", 30, 333, 4, True), ("gnn", 24, 1000, 5, False)])
def test_gnn_period_kernel_with_edge_tiles_in_global_scratch(workload, stores, n, T, train):
    """Round 6: graphs whose embeddings do not fit in LDS (3 x 16 dense: 19 nodes + 70 edges; one warehouse with 24 / 30 stores: up to
    31 + 62) run the period kernel with the EDGE tiles in a per-workgroup scratch area in global memory (`nic_gnn_period_ok` = 2) -
    the one-warehouse ones with the allocation + env step fused behind, as on small graphs.  Against the per-MLP launches."""
    from neural_inventory_control_amd import workloads
    setting, policy, _, _, _ = workloads.get(workload)
    if stores != setting["problem_params"]["n_stores"]:
        setting["problem_params"]["n_stores"] = stores
    a, b = _gnn_run_pair(setting, policy, n, T, 5, train=train, use_period_kernel=(True, False), use_period_bwd=(False, False))
    assert a["eng"]._period and a["eng"].edge_scratch is not None and not b["eng"]._period
    assert any("spill" in k for _, k in a["eng"].timer.order), sorted({k for _, k in a["eng"].timer.order})
    assert abs(a["total"] - b["total"]) <= 2e-6 * abs(b["total"]) and abs(a["rep"] - b["rep"]) <= 2e-6 * abs(b["rep"])
    torch.testing.assert_close(a["rewards"], b["rewards"], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(a["state"], b["state"], rtol=1e-5, atol=1e-4)
    for x, y in zip(a["grads"], b["grads"]):
        assert float((x - y).norm()) <= 1e-5 * float(y.norm()) + 1e-9


def test_gnn_period_backward_differential_fuzz():
    """... and on random settings: 2-16 stores on one warehouse, 2-3 warehouses with random (connected) adjacency, pipelines of 2-9 /
    2-5 slots, transshipment, edge costs, 17-300 scenarios."""
    import random
    from neural_inventory_control_amd import workloads
    rng = random.Random(20261004)
    done = 0
    for trial in range(10):
        many = trial % 3 == 2
        setting, policy, _, _, _ = workloads.get("gnn_many_warehouses" if many else "gnn")
        if many:
            S, Wn = rng.choice([4, 7, 16]), setting["problem_params"]["n_warehouses"]
            setting["problem_params"]["n_stores"] = S
            adj = [[1 if (w == 0 or rng.random() < 0.6) else 0 for _ in range(S)] for w in range(Wn)]
            adj[0] = [1] * S
            adj[1][0] = adj[2][0] = 1                      # some store sees every warehouse (GnnRollout.supports)
            setting["problem_params"]["warehouse_store_adjacency"] = adj
            for k in ("lead_time",):
                if isinstance(setting["store_params"][k].get("value"), list):
                    setting["store_params"][k]["value"] = [[rng.randint(1, 6) for _ in range(Wn)] for _ in range(S)]
        else:
            S = rng.choice([2, 3, 5, 9, 12, 16])
            Ws, wlead = rng.randint(2, 9), rng.randint(2, 5)
            setting["problem_params"]["n_stores"] = S
            setting["store_params"]["lead_time"] = {"sample_across_stores": True, "vary_across_samples": False, "expand": False,
                                                    "range": [1, Ws + 1]}
            setting["store_params"]["initial_inventory"]["inventory_periods"] = Ws
            setting["warehouse_params"]["lead_time"] = wlead
            if rng.random() < 0.5:
                setting["warehouse_params"]["edge_cost"] = 0.7
            policy["transshipment"] = rng.random() < 0.4
        n, T = rng.randint(17, 300), rng.randint(3, 6)
        try:
            pair = _gnn_run_pair(setting, policy, n, T, trial, use_period_bwd=(True, False))
        except (KeyError, ValueError, IndexError) as e:     # (a store-parameter list the mutated store count does not match)
            if many:
                continue
            raise
        if pair is None:
            continue
        a, b = pair
        assert a["eng"]._period_bwd and not b["eng"]._period_bwd
        _assert_same_gradients(a, b, tag=dict(trial=trial, many=many, S=S, n=n, T=T))
        done += 1
    assert done >= 6


@pytest.mark.parametrize("setting_name", ["cfg3", "cfg2"])
def test_per_sample_cost_tables_with_shuffled_batches_follow_the_oracle(setting_name):
    """`vary_across_samples: True` (data_handling.py:258-259): underage costs differ per SCENARIO, so every shuffled batch has
    its own cost table.  The engines cache the compacted tables per presented tensors; entries pin those tensors, so a later
    batch that lands on a recycled address cannot inherit another batch's costs.  Every batch of two shuffled epochs is
    checked against the oracle on the fused per-period route (cfg3), the whole-horizon route (cfg2) and the Simulator route."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from oracle import inventory_oracle as orc
    setting, policy, _, _, _ = workloads.get(setting_name)
    if setting_name == "cfg3":
        setting["problem_params"]["n_stores"] = 4
        policy["neurons_per_hidden_layer"]["master"] = [32, 32]
    setting["store_params"]["underage_cost"] = {"sample_across_stores": False, "vary_across_samples": True, "expand": False,
                                                "range": [4.0, 14.0]}
    obs = defaultdict(lambda: None, setting["observation_params"])
    T, n, bs = 12, 96, 32
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, dict(setting["seeds"]))
    ds = DatasetCreator().create_datasets(sc, split=False)
    assert float(ds.data["underage_costs"].std(dim=0).max()) > 0.5  # really per-sample
    torch.manual_seed(5)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    S = setting["problem_params"]["n_stores"]
    F = S * ds.data["initial_inventories"].shape[2] + (ds.data["initial_warehouse_inventories"].shape[2] if "initial_warehouse_inventories" in ds.data and policy["name"] != "vanilla_one_store" else 0)
    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(F)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    pol = orc.policy_from_state_dict(policy, state, setting["problem_params"],
                                     model.warehouse_upper_bound.cpu() if torch.is_tensor(model.warehouse_upper_bound) else None)
    loader = DeviceBatches(ds, bs, shuffle=True, device=DEV, seed=3)
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    tr.use_fused_rollout = False
    checked = 0
    for _epoch in range(2):
        for batch in loader:
            cpu = {k: v.cpu() for k, v in batch.items()}
            with torch.no_grad():
                ref = orc.rollout(pol, T, setting["problem_params"], cpu, obs, 0)
                t_fused, _ = eng.run(batch, T, 0, train=False, observation_params=obs)
                t_sim, _ = tr.simulate_batch(PolicyLoss(), sim, model, T, setting["problem_params"], batch, obs, 0, False)
            assert abs(float(t_fused) - float(ref.total)) <= 1e-5 * abs(float(ref.total)), (checked, "fused")
            assert abs(float(t_sim) - float(ref.total)) <= 1e-5 * abs(float(ref.total)), (checked, "simulator")
            per = eng.per_period_rewards().sum(dim=0).cpu()
            assert float(((per - ref.per_period.sum(dim=0)).abs() / ref.per_period.sum(dim=0).abs().clamp_min(1e-9)).max()) <= 1e-5
            checked += 1
            del batch  # let the allocator recycle the batch's storage for the next one
    assert checked == 6


# ---- the symmetry-aware policy BASELINE cfg3 names (not in the reference's source; parity UNPINNED) -------------------

@pytest.mark.parametrize("n_stores", [5, 16])
def test_symmetry_aware_policy_matches_its_cpu_restatement(n_stores):
    """`symmetry_aware` on the generic route (Simulator.step as a HIP kernel per period + HipLinear layers shared over the stores)
    against this repository's own CPU restatement (oracle.symmetry_aware_act): per-period rewards, total cost at 1e-5, parameter
    gradients at 2e-5.  There is no upstream implementation to compare with - the oracle follows SURVEY 2.2's recovery."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from oracle import inventory_oracle as orc
    setting, policy, _, _, _ = workloads.get("cfg3_symmetry_aware")
    setting["problem_params"]["n_stores"] = n_stores
    B, T = 37, 9
    obs = defaultdict(lambda: None, setting["observation_params"])
    data = orc.generate_scenario_data(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"],
                                      setting["echelon_params"], B, obs, setting["seeds"])

    class _Sc:
        problem_params = setting["problem_params"]
        store_params = setting["store_params"]
    torch.manual_seed(11)
    model = NeuralNetworkCreator().create_neural_network(_Sc(), policy, device=DEV)
    sim, tr = Simulator(device=DEV), Trainer(device=DEV)
    dev_data = {k: v.to(DEV) for k, v in data.items()}
    with torch.no_grad():   # materialise the lazy layers
        o, _ = sim.reset(T, setting["problem_params"], dict(dev_data), obs)
        model(o)
    total, rep = tr.simulate_batch(PolicyLoss(), sim, model, T, setting["problem_params"], dict(dev_data), obs, 3, False)
    (total / (B * T * n_stores)).backward()
    torch.cuda.synchronize()
    pol = orc.policy_from_state_dict(policy, {k: v.detach().cpu() for k, v in model.state_dict().items()},
                                     setting["problem_params"], model.warehouse_upper_bound.cpu())
    res, _, grads = orc.train_step_gradients(pol, T, setting["problem_params"], data, obs, 3)
    assert abs(float(total) - float(res.total)) <= 1e-5 * abs(float(res.total))
    assert abs(float(rep) - float(res.reported)) <= 1e-5 * abs(float(res.reported))
    named = dict(model.named_parameters())
    for key, gref in zip(pol.param_keys(), grads):
        assert _rel(named[key].grad, gref) <= GRAD_TOL, key


def test_small_route_step_caches_follow_their_inputs():
    """The small route skips three launches while their inputs are unchanged (initial-state copies, the d loss / d reward fill).
    What must invalidate them does: an in-place change of the presented initial inventories, a new tensor, a different gradient
    scale, a different batch size - each compared with a fresh engine."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    setting, policy, _, _, _ = workloads.get("cfg4")
    obs = defaultdict(lambda: None, setting["observation_params"])
    T, n = 9, 200
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, setting["seeds"])
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    torch.manual_seed(11)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    F = sum(int(np.prod(data[k].shape[1:])) for k in ("initial_inventories", "initial_warehouse_inventories",
                                                        "initial_echelon_inventories") if k in data)

    def fresh(d, scale):
        e = FusedRollout(model, setting["problem_params"], DEV)
        e.materialize(F)
        tot, _ = e.run(d, T, 0, train=True, observation_params=obs, grad_scale=scale)
        return float(tot), [p.grad.clone() for p in model.parameters()]

    eng = FusedRollout(model, setting["problem_params"], DEV)
    eng.materialize(F)

    def same(d, scale):
        tot, _ = eng.run(d, T, 0, train=True, observation_params=obs, grad_scale=scale)
        got = (float(tot), [p.grad.clone() for p in model.parameters()])
        want = fresh(d, scale)
        assert got[0] == want[0]
        for a, b in zip(got[1], want[1]):
            assert torch.equal(a, b)
        return got

    first = same(data, 1e-3)
    assert eng.small is not None
    again = same(data, 1e-3)                       # (everything cached)
    assert again[0] == first[0]
    data["initial_inventories"].mul_(1.5)          # in place: same tensor object, new version
    changed = same(data, 1e-3)
    assert changed[0] != first[0]
    d2 = dict(data)
    d2["initial_warehouse_inventories"] = data["initial_warehouse_inventories"] + 3.0   # a new tensor
    assert same(d2, 1e-3)[0] != changed[0]
    scaled = same(d2, 2e-3)                         # a different gradient scale
    for a, b in zip(scaled[1], same(d2, 1e-3)[1]):
        torch.testing.assert_close(a, 2.0 * b, rtol=1e-6, atol=0)
    same({k: v[:77].contiguous() for k, v in d2.items()}, 1e-3)   # a smaller batch (padding columns must be zero again)


@pytest.mark.parametrize("S,Wn,seed", [(5, 2, 1), (10, 3, 2), (21, 4, 3), (64, 3, 4), (17, 2, 5)])
def test_compact_logit_rows_through_the_fused_head_env_launches_on_random_graphs(S, Wn, seed):
    """Sparse many-warehouse graphs drawn at random (every store served by one or two warehouses; store counts that do not fill the
    four lanes of a scenario; a warehouse that may end up with a single store): the fused head + env launches on the COMPACT
    logits (`nic_head_env_fwd` / `_bwd` with `logit_rows`: only connected (store, warehouse) pairs have a logit row) against the separate
    head and env launches on the scattered [S * Wn + Wn] layout - rewards, states, orders and parameter gradients bit for bit."""
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    setting = workloads.many_warehouses(min(S, 64), min(Wn, 3), seed=seed) if Wn <= 3 else None
    if setting is None:   # (the builder's cost lists stop at three warehouses)
        import random
        rnd = random.Random(seed)
        setting = workloads.many_warehouses(S, 3, seed=seed)
        adj = [[0] * S for _ in range(Wn)]
        lead = [[0] * Wn for _ in range(S)]
        for s_ in range(S):
            for w in rnd.sample(range(Wn), rnd.choice([1, 2])):
                adj[w][s_], lead[s_][w] = 1, rnd.randint(1, 6)
        setting["problem_params"].update({"n_warehouses": Wn, "warehouse_store_adjacency": adj})
        setting["store_params"]["lead_time"] = workloads._const(lead)
        setting["warehouse_params"] = {"holding_cost": [0.3, 0.4, 0.2, 0.35][:Wn], "lead_time": 3,
                                       "edge_cost": [0.5, 1.5, 0.7, 0.9][:Wn]}
    policy = workloads.get("cfg5")[1]
    import copy
    policy = copy.deepcopy(policy)
    policy["output_sizes"]["master"] = S * Wn + Wn
    policy["neurons_per_hidden_layer"]["master"] = [64, 64]
    obs = defaultdict(lambda: None, setting["observation_params"])
    T, n = 7, 150
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"],
                  n, obs, setting["seeds"])
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    out = {}
    for fuse in (True, False):
        torch.manual_seed(21)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng = FusedRollout(model, setting["problem_params"], DEV)
        eng.fuse_head_env = fuse
        eng.materialize(eng.input_rows(data, obs))
        total, _ = eng.run(data, T, 0, train=True, observation_params=obs)
        torch.cuda.synchronize()
        assert eng.small is None and eng.horizon is None
        compact = eng.live_rows is not None
        out[fuse] = (float(total), eng.per_period_rewards().clone(), eng.states.clone(), eng.orders.clone(),
                     [p.grad.clone() for p in model.parameters()], compact)
    a, b = out[True], out[False]
    assert a[5] and b[5], "the graph was meant to be sparse enough for the compact logits layer"
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    for x, y in zip(a[4], b[4]):
        assert torch.equal(x, y)
    assert all(bool(torch.isfinite(g_).all()) for g_ in a[4])


# ---- round 5: the fused per-period tail (csrc/period_tail.hip) ---------------------------------------------------------------
TAIL_CASES = ["cfg3_one_warehouse_16_vanilla", "cfg3_one_warehouse_5_vanilla", "x_transshipment_backlogged_vanilla"]


def _run_engine(model, pp, data, T, ignore, obs, fuse_tail, train=True):
    from neural_inventory_control_amd.rollout import KernelTimer
    eng = FusedRollout(model, pp, DEV)
    eng.fuse_tail = fuse_tail
    eng.materialize(eng.input_rows(data, obs))
    eng.timer = KernelTimer(record_order=True)
    total, rep = eng.run(data, T, ignore, train=train, observation_params=obs)
    torch.cuda.synchronize()
    tags = {t for t, _ in eng.timer.order}
    return eng, float(total), float(rep), tags


@pytest.mark.parametrize("name", TAIL_CASES)
def test_fused_tail_launches_on_the_warehouse_fixtures(name):
    """Round 5 (csrc/period_tail.hip): the fixtures whose shapes the fused tail takes (<= 16 stores, <= 32 logits, <= 51 state rows)
    run it by default - forward: logits layer + head + env step + next period's first layer in ONE launch; backward: first layer's
    input gradient + env / head adjoints + logits layer backward in ONE launch.  Against the separate launches: rewards, orders and
    states agree to fp32 round-off of the two GEMM stages (the tail carries the first layer's bias inside the contraction and splits
    the logits contraction over four wavefronts; at these widths the separate launches do neither), gradients <= 1e-5; against the
    reference's golden numbers: the usual bars."""
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    out = {}
    for fuse in (True, False):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.materialize(eng.input_rows(data, c["observation_params"]))
        _load(model, g)
        eng, total, rep, tags = _run_engine(model, c["problem_params"], data, c["periods"], c["ignore"], c["observation_params"], fuse)
        assert ("tail_fwd" in tags and "tail_bwd" in tags and "head_env_fwd" not in tags and "head_env_bwd" not in tags) == fuse, tags
        out[fuse] = (total, rep, eng.per_period_rewards().clone(), eng.states.clone(), eng.orders.clone(),
                     [p.grad.clone() for p in model.parameters()])
        if fuse:
            _check_grads(model, g, GRAD_TOL)
            exp = _Expected(g, c)
            assert abs(total - exp.total) <= 1e-5 * abs(exp.total) and abs(rep - exp.reported) <= 1e-5 * abs(exp.reported)
            torch.testing.assert_close(eng.per_period_rewards().cpu(), exp.rewards, rtol=1e-5, atol=1e-5)
    a, b = out[True], out[False]
    assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0]) and abs(a[1] - b[1]) <= 2e-6 * abs(b[1])
    torch.testing.assert_close(a[2], b[2], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a[3], b[3], **STATE_TOL)
    torch.testing.assert_close(a[4], b[4], **STATE_TOL)
    for x, y in zip(a[5], b[5]):
        assert float((x - y).norm()) <= 1e-5 * float(y.norm()) + 1e-12


@pytest.mark.parametrize("n,T,hidden", [(100, 5, [256, 256, 256]), (24, 4, [512, 512]), (2048 + 17, 3, [256, 512])])
def test_fused_tail_is_bit_identical_to_the_separate_launches_where_they_take_the_same_contraction_order(n, T, hidden):
    """BASELINE cfg3's setting (16 stores, 51 state rows, 17 logits) with hidden layers >= 256 wide at small batches: there the
    separate launches are thin_in_fwd (bias inside the contraction), gemm_wx_stream_kernel<1, 4> (logits / first layer's input
    gradient: contraction split over four wavefronts) and thin_bwd - exactly the arithmetic the tail kernels restate.  Per-period
    rewards, states, orders, logits, hidden activations, the pre-activation gradient histories and every hidden layer's weight
    gradient are BIT-IDENTICAL; the logits layer's weight gradient is summed per workgroup instead of per scenario split: 1e-6.
    Ragged batches (100 = three blocks + 4 scenarios; 2,065: more blocks than a group)."""
    import copy
    from neural_inventory_control_amd import workloads
    from collections import defaultdict
    setting, policy, _, _, _ = workloads.get("cfg3")
    policy = copy.deepcopy(policy)
    policy["neurons_per_hidden_layer"]["master"] = list(hidden)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                  obs, setting["seeds"], sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    out = {}
    for fuse in (True, False):
        torch.manual_seed(11)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng, total, rep, tags = _run_engine(model, setting["problem_params"], data, T, 0, obs, fuse)
        assert ("tail_fwd" in tags) == fuse and ("tail_bwd" in tags) == fuse, tags
        out[fuse] = (total, eng.per_period_rewards().clone(), eng.states.clone(), eng.orders.clone(), eng.logits.clone(),
                     [h.clone() for h in eng.hidden], [h.clone() for h in eng.dZhist], [p.grad.clone() for p in model.parameters()])
    a, b = out[True], out[False]
    if n <= 1024:   # (beyond that the separate logits GEMM takes the LDS-DMA kernel: one wavefront per contraction)
        assert a[0] == b[0]
        for x, y in zip(a[1:5], b[1:5]):
            assert torch.equal(x, y)
        for x, y in zip(a[5] + a[6], b[5] + b[6]):
            assert torch.equal(x, y)
        for x, y in zip(a[7][:-2], b[7][:-2]):
            assert torch.equal(x, y)
    else:
        assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0])
        torch.testing.assert_close(a[1], b[1], rtol=1e-5, atol=1e-5)
    for x, y in zip(a[7], b[7]):
        assert float((x - y).norm()) <= 2e-6 * float(y.norm()) + 1e-12


def test_fused_tail_evaluation_without_history_and_discrete_allocation_falls_back():
    """Evaluation through the tail without the state / order history (two rolling state blocks), and discrete allocation
    (orders rounded between head and env step) keeping the separate launches."""
    g = Golden("cfg3_one_warehouse_16_vanilla")
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    res = {}
    for hist in (True, False):
        model = _model(g, c)
        eng = FusedRollout(model, c["problem_params"], DEV)
        eng.eval_history = hist
        eng.materialize(eng.input_rows(data, c["observation_params"]))
        _load(model, g)
        with torch.no_grad():
            total, _ = eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
        assert eng._use_tail()
        res[hist] = (float(total), eng.per_period_rewards().clone(), {k: v.clone() for k, v in eng.final_state().items()})
    assert res[True][0] == res[False][0] and torch.equal(res[True][1], res[False][1])
    for k in res[True][2]:
        assert torch.equal(res[True][2][k], res[False][2][k])
    with torch.no_grad():
        eng.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"], discrete_allocation=True)
    assert not eng._use_tail()


def test_step_graph_guard_sees_the_stream_hazard_on_this_torch_build():
    """`use_step_graph = "auto"` only captures training steps when this torch build REPORTS the condition under which a capture
    must be refused (an autograd graph alive on another stream): the guard's self-test builds that condition on a dummy
    parameter and must see the report - recognised by its origin (torch/autograd) or the node it names, not by one sentence."""
    Trainer._hazard_guard.clear()
    assert Trainer._stream_hazard_is_reported(DEV) is True
    assert Trainer._stream_hazard_is_reported("cpu") is False


# ---- round 5: the whole-horizon forward of the wide policy - since round 6 an EXPERIMENT outside the default library
# (tools/experiments/wide_rollout.hip, include/nic_experiments.h): these tests run against a library built with NIC_BUILD_EXPERIMENTS=1
def _needs_experiments():
    if not torch.cuda.is_available():
        return True
    try:
        return not _lib.has_experiments()
    except Exception:
        return True


needs_experiments = pytest.mark.skipif(_needs_experiments(), reason="experimental entry points: build with NIC_BUILD_EXPERIMENTS=1")


@needs_experiments
@pytest.mark.parametrize("n,T,hidden", [(100, 5, [512, 512, 512]), (2048 + 17, 3, [512, 512]), (8192, 4, [512, 512, 512])])
def test_wide_whole_horizon_forward_matches_the_per_period_route(n, T, hidden):
    """BASELINE cfg3's setting with 512-wide hidden layers: ALL periods in one forward launch (a workgroup carries 32 scenarios
    through the horizon; weights streamed as packed MFMA fragments, activations in LDS, logits from the accumulators) against the
    per-period launches: per-period rewards / per-scenario totals <= 1e-5, states and orders to the usual state tolerance, hidden
    activation and logit histories <= 1e-5, and - the backward sweep running on the histories the kernel left - gradients
    <= 1e-5 per parameter tensor.  Ragged batches (100 = three blocks + 4; 2,065), one block per CU (8,192)."""
    import copy
    from collections import defaultdict
    from neural_inventory_control_amd import workloads
    from neural_inventory_control_amd.rollout import KernelTimer
    setting, policy, _, _, _ = workloads.get("cfg3")
    policy = copy.deepcopy(policy)
    policy["neurons_per_hidden_layer"]["master"] = list(hidden)
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n,
                  obs, setting["seeds"], sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    out = {}
    for wide in (True, False):
        torch.manual_seed(11)
        model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        eng = FusedRollout(model, setting["problem_params"], DEV)
        eng.use_wide = wide
        eng.materialize(eng.input_rows(data, obs))
        eng.timer = KernelTimer(record_order=True)
        total, rep = eng.run(data, T, 0, train=True, observation_params=obs)
        torch.cuda.synchronize()
        tags = {t for t, _ in eng.timer.order}
        assert ("wide_fwd" in tags) == wide, tags
        out[wide] = (float(total), eng.per_period_rewards().clone(), eng.states.clone(), eng.orders.clone(), eng.logits.clone(),
                     [h_.clone() for h_ in eng.hidden], [p.grad.clone() for p in model.parameters()])
    a, b = out[True], out[False]
    assert abs(a[0] - b[0]) <= 2e-6 * abs(b[0])
    tot_a, tot_b = a[1].sum(0), b[1].sum(0)
    assert float(((tot_a - tot_b).abs() / tot_b.abs().clamp_min(1e-9)).max()) <= 1e-5
    torch.testing.assert_close(a[1], b[1], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a[2], b[2], **STATE_TOL)
    torch.testing.assert_close(a[3], b[3], **STATE_TOL)
    torch.testing.assert_close(a[4][:, :, :n], b[4][:, :, :n], rtol=1e-4, atol=1e-4)
    for x, y in zip(a[5], b[5]):
        torch.testing.assert_close(x[:, :, :n], y[:, :, :n], rtol=1e-4, atol=1e-4)
    for x, y in zip(a[6], b[6]):
        assert float((x - y).norm()) <= 1e-5 * float(y.norm()) + 1e-12
