"""`nic_closed_form_sweep` (csrc/closed_form.hip: K candidate level vectors per launch, a small group of candidates per lane) on the
device: every candidate's per-chain totals and per-wavefront partial rows EQUAL those of a single-candidate launch of
`nic_closed_form_rollout_sums` with that candidate's levels; `ClosedFormRollout.sweep` and `nic::sweep_closed_form` on top."""
import copy
import functools
from collections import defaultdict

import pytest
import torch

import closed_form_checks as cfc
import closed_form_sweep_checks as swc
from neural_inventory_control_amd import _lib, closed_form, library, workloads
from neural_inventory_control_amd.closed_form import ClosedFormRollout
from neural_inventory_control_amd.data_handling import Scenario
from neural_inventory_control_amd.layout import EnvProblem
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _last_kernel():
    return (_lib.lib().nic_last_kernel() or b"").decode()


@functools.lru_cache(maxsize=None)
def _golden(name):
    """(case, the 9 candidate rows every K takes its first rows from, single-launch references per (row, want_grad))"""
    case = swc.golden_case(name, DEV)
    levels = case.candidates(swc.SCALES_9)
    return case, levels, {(k, wg): swc.hip_single(case, levels[k].contiguous(), wg) for k in range(9) for wg in (True, False)}


@pytest.mark.parametrize("K", [1, 5, 9])
@pytest.mark.parametrize("name", cfc.CLOSED_FORM_CASES)
def test_sweep_equals_single_launches_on_golden_cases(name, K):
    """chain_totals[k] and partial[k] (row for row) of the sweep against the single launch with levels[k], with and without
    gradients; padding columns of chain_totals are not written."""
    case, all_levels, refs = _golden(name)
    levels = all_levels[:K].contiguous()
    totals, _ = swc.assert_sweep_equals_singles(
        case, levels, lambda lv, wg: _padding_checked(case, lv, wg), lambda k, wg: refs[(k, wg)])
    assert _last_kernel().startswith("closed_form_sweep_kernel<0,")   # (the forward-only launch came last)
    g = case.golden   # row 2 = the fixture's own levels
    if K > 2:
        assert abs(float(totals[2, 0, :, :case.B].double().sum()) - float(g.z["total"])) <= 1e-6 * abs(float(g.z["total"]))


def _padding_checked(case, levels, want_grad):
    totals, part = swc.hip_sweep(case, levels, want_grad, fill=-7.0)
    assert bool((totals[..., case.B:] == -7.0).all())
    totals[..., case.B:] = 0.0   # (the single launches' buffers start as zeros)
    return totals, part


def _workload_case(which):
    """n = 200 chains, T = 13: settings that reach the kernel variants the fixtures do not."""
    s = workloads.one_store(lost=False, poisson=False)
    policy, levels = "base_stock", [21.5]
    if which == "per_scenario_leads":     # lead-time table with a scenario stride: the generic store kernel (WC = 0)
        s["store_params"]["lead_time"] = {"sample_across_stores": False, "vary_across_samples": True, "range": [2, 5]}
        policy, levels = "capped_base_stock", [23.0, 6.5]
    elif which == "long_pipeline":        # 6 slots: MF = 8
        s["store_params"]["lead_time"] = workloads._const(6)
        levels = [33.0]
    elif which == "three_stores":         # grid.y = 3
        s["problem_params"]["n_stores"] = 3
        s["store_params"]["demand"].update(mean=[5.0, 3.0, 6.0], std=[1.6, 1.0, 2.0], correlation=0.3)
        s["store_params"]["lead_time"] = workloads._per_store(2, 5)
    elif which == "lost_profit":
        s["problem_params"].update(lost_demand=True, maximize_profit=True)
        policy, levels = "capped_base_stock", [22.0, 7.0]
    obs = defaultdict(lambda: None, s["observation_params"])
    sc = Scenario(13, s["problem_params"], copy.deepcopy(s["store_params"]), None, None, 200, obs, dict(s["seeds"]))
    return swc.make_case(s["problem_params"], sc.get_data(), policy, 13, 3, torch.tensor(levels), DEV)


@pytest.mark.parametrize("which,kernel", [("per_scenario_leads", "closed_form_sweep_kernel<2,4,false,0,"),
                                          ("long_pipeline", "closed_form_sweep_kernel<1,8,false,0,"),
                                          ("three_stores", "closed_form_sweep_kernel<1,4,false,4,"),
                                          ("lost_profit", "closed_form_sweep_kernel<2,4,false,4,")])
def test_sweep_equals_single_launches_on_other_variants(which, kernel):
    case = _workload_case(which)
    levels = case.candidates(swc.SCALES_5)
    swc.hip_sweep(case, levels, True)
    assert _last_kernel().startswith(kernel), _last_kernel()
    if which == "three_stores":
        assert case.prob.S == 3
    swc.assert_sweep_equals_singles(case, levels, lambda lv, wg: swc.hip_sweep(case, lv, wg),
                                    lambda k, wg: swc.hip_single(case, levels[k].contiguous(), wg))
    # discrete allocation: forward only
    got, ref = swc.hip_sweep(case, levels, False, round_orders=True), [swc.hip_single(case, levels[k].contiguous(), False, True) for k in range(5)]
    for k in range(5):
        assert torch.equal(got[0][k], ref[k][0]) and torch.equal(got[1][k], ref[k][1])
    assert not torch.equal(got[0], swc.hip_sweep(case, levels, False)[0])


def _engine(wl):
    """(engine, data, T, demand trace, candidate rows [5][L]) of a closed-form workload at 500 scenarios x 12 periods"""
    setting, policy, _, _, _ = workloads.get("echelon_stock" if wl == "echelon_stock" else "base_stock")
    if wl == "capped_base_stock":
        policy = workloads._closed_form("capped_base_stock", 2)
    obs = defaultdict(lambda: None, setting["observation_params"])
    n, T = 500, 12
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], n, obs,
                  dict(setting["seeds"]), sampler="hip", device=DEV)
    data = {k: v.to(DEV) for k, v in sc.get_data().items()}
    torch.manual_seed(5)
    model = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
    eng = ClosedFormRollout(model, setting["problem_params"], DEV)
    with torch.no_grad():
        base = model.closed_form_levels().detach().clone()
    if wl == "capped_base_stock":
        base = base * torch.tensor([2.2, 0.7], device=DEV)   # (softplus(10) twice: a level the cap binds under)
    levels = (base[None, :] * torch.tensor(swc.SCALES_5, device=DEV)[:, None]).contiguous()
    return eng, setting, data, T, sc.demands_soa, levels


@pytest.mark.parametrize("wl", ["base_stock", "capped_base_stock", "echelon_stock"])
def test_engine_sweep_matches_a_loop_of_run(wl):
    """`ClosedFormRollout.sweep` against `run` once per row (the row fed in as the model's levels): totals and reported costs at 1e-6,
    level gradients at 1e-5 of their norm (the last sum over wavefronts may be taken in another order); discrete allocation
    forward only; the operator returns the engine's numbers."""
    eng, setting, data, T, trace, levels = _engine(wl)
    eng.keep_chain_totals = True
    kw = dict(observation_params=setting["observation_params"], demand_soa=trace)
    total, reported, grad = eng.sweep(levels, data, T, 3, **kw)
    assert _last_kernel().startswith("closed_form_sweep_kernel<")
    assert tuple(total.shape) == (5,) and tuple(reported.shape) == (5,) and tuple(grad.shape) == tuple(levels.shape)
    assert bool((eng.sweep_totals[..., eng.prob.B:] == 0).all())
    t0, r0, g0 = eng.sweep(levels, data, T, 3, want_grad=False, **kw)
    assert g0 is None and torch.equal(t0, total) and torch.equal(r0, reported)
    td, rd, _ = eng.sweep(levels, data, T, 3, want_grad=False, discrete_allocation=True, **kw)
    for k in range(5):
        row = levels[k].clone().requires_grad_()
        eng.model.closed_form_levels = lambda row=row: row
        t, r = eng.run(data, T, 3, train=True, **kw)
        t.backward()
        assert abs(float(total[k]) - float(t)) <= 1e-6 * abs(float(t))
        assert abs(float(reported[k]) - float(r)) <= 1e-6 * abs(float(r))
        assert float((grad[k] - row.grad).norm()) <= 1e-5 * float(row.grad.norm())
        with torch.no_grad():
            t, r = eng.run(data, T, 3, train=False, discrete_allocation=True, **kw)
        assert abs(float(td[k]) - float(t)) <= 1e-6 * abs(float(t)) and abs(float(rd[k]) - float(r)) <= 1e-6 * abs(float(r))
    assert not torch.equal(td, total)
    # the registered operator: same launch, same numbers
    prob = EnvProblem(setting["problem_params"], data, torch.device(DEV))
    h = library.register_problem(prob)
    state0 = closed_form.pack_state0(data, prob)
    pid = closed_form.POLICY_ID[eng.name]
    t2, r2, g2 = torch.ops.nic.sweep_closed_form(levels, trace, state0, h, pid, T, 0, 3, False, True)
    assert torch.equal(t2, total) and torch.equal(r2, reported) and torch.equal(g2, grad)
    t3, r3, g3 = torch.ops.nic.sweep_closed_form(levels, trace, state0, h, pid, T, 0, 3, True, False)
    assert torch.equal(t3, td) and torch.equal(r3, rd) and not bool(g3.any())
    # (no autograd formula is registered for this operator, so the autograd-registration check has nothing to look at)
    torch.library.opcheck(torch.ops.nic.sweep_closed_form, (levels, trace, state0, h, pid, T, 0, 3, False, True),
                          test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
    library.release_problem(h)


def test_sweep_refuses_bad_arguments_before_launching():
    case = swc.golden_case(cfc.CLOSED_FORM_CASES[1], DEV)
    levels = case.candidates(swc.SCALES_5)
    swc.hip_single(case, levels[0].contiguous(), True)
    before = _last_kernel()
    assert before.startswith("closed_form_kernel<")
    lib, L = _lib.lib(), levels.shape[1]
    part = torch.zeros(5, lib.nic_closed_form_num_partials(case.B, case.prob.S), L + 2, device=DEV)
    stream = _lib.current_stream()
    for args, msg in (((case.desc(levels[0]), levels.data_ptr(), 0, None, part.data_ptr(), L + 2, 1, stream), "at least one candidate"),
                      ((case.desc(levels[0]), None, 5, None, part.data_ptr(), L + 2, 1, stream), "null levels"),
                      ((case.desc(levels[0]), levels.data_ptr(), 5, None, None, L + 2, 1, stream), "partial buffer missing"),
                      ((case.desc(levels[0]), levels.data_ptr(), 5, None, part.data_ptr(), L + 1, 1, stream), "rows too short"),
                      ((case.desc(levels[0], True), levels.data_ptr(), 5, None, part.data_ptr(), L + 2, 1, stream), "no gradient")):
        with pytest.raises(_lib.NicError, match=msg):
            _lib.check(lib.nic_closed_form_sweep(*args))
        assert _last_kernel() == before
    torch.cuda.synchronize()
    assert not bool(part.any())   # nothing ran


def test_engine_sweep_raises_like_run():
    eng, setting, data, T, trace, levels = _engine("base_stock")
    kw = dict(observation_params=setting["observation_params"], demand_soa=trace)
    with pytest.raises(ValueError, match="discrete_allocation"):
        eng.sweep(levels, data, T, 3, discrete_allocation=True, **kw)
    with pytest.raises(ValueError, match="greater than the number of periods"):
        eng.sweep(levels, data, T + 1, 3, **kw)
    with pytest.raises(ValueError, match="levels must be"):
        eng.sweep(levels.reshape(1, 5), data, T, 3, **kw)
    echelon = ClosedFormRollout(eng.model, setting["problem_params"], DEV)
    echelon.name = "echelon_stock"   # a one-store setting is outside the chain kernel
    with pytest.raises(ValueError, match="outside the fused closed-form kernel"):
        echelon.sweep(levels, data, T, 3, **kw)
