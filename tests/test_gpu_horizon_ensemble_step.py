"""`HorizonPolicyEnsemble` beyond the launch pair: the model-batched GEMM route against the per-model loop, bound parameters,
`train_step` / `fit` with an `EnsembleAdam`, on the three real-data data_driven fixtures with K = 3.

Routes that must run the same arithmetic are held to bit equality (batched GEMMs against the loop, `train_step` against `run` +
`optimizer.step` on a twin, `fit` against its hand-written loop); against `torch.optim.Adam` the bar is the referee of
test_gpu_ensemble_adam.py (`_referee`: our error against ensemble_adam_checks.adam_f64 at most 2 x torch's own)."""
import copy

import numpy as np
import pytest
import torch

import test_gpu_horizon_ensemble as base   # _models: a fixture's policy + two more seeds on the device
from golden_io import Golden
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
from neural_inventory_control_amd.horizon_ensemble import HorizonPolicyEnsemble, layer_slices
from neural_inventory_control_amd.rollout import FusedRollout
from test_gpu_ensemble_adam import _referee

pytestmark = pytest.mark.gpu
DEV = base.DEV
K = 3
LRS = (1e-3, 3e-3, 1e-2)


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class _Setting:
    def __init__(self, name):
        self.g = Golden(name)
        self.c = self.g.fresh_config()
        self.data = {k: v.to(DEV) for k, v in self.g.data.items()}
        self.T, self.ignore, self.obs = self.c["periods"], self.c["ignore"], self.c["observation_params"]

    def engine(self, bound=True, model_gemms=True):
        models = base._models(self.g, self.g.fresh_config())
        ens = HorizonPolicyEnsemble(models, self.c["problem_params"], DEV)
        ens.model_gemms = model_gemms
        if bound:
            ens.bind_parameters()
        return ens

    def optimizer(self, ens, lrs=LRS):
        return EnsembleAdam(ens.n_models, ens.weights.shape[1], DEV, lr=list(lrs), param_shapes=ens.param_shapes)

    def run(self, ens, data=None, periods=None, **kw):
        return ens.run(data or self.data, periods or self.T, self.ignore, observation_params=self.obs, **kw)

    def step(self, ens, opt, data=None, periods=None):
        return ens.train_step(data or self.data, periods or self.T, self.ignore, opt, self.obs)


_SETTINGS = {}


def _setting(name):
    if name not in _SETTINGS:
        _SETTINGS[name] = _Setting(name)
    return _SETTINGS[name]


def _packed(models):
    return torch.stack([torch.cat([p_.detach().reshape(-1) for lin in m.master_linears() for p_ in (lin.weight, lin.bias)]) for m in models])


# ---- routes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", base.ENGINE_CASES)
def test_batched_gemms_give_the_bits_of_the_per_model_loop(name):
    s = _setting(name)
    a, b = s.engine(bound=False, model_gemms=True), s.engine(bound=False, model_gemms=False)
    for train in (False, True):
        ta, tb = s.run(a, train=train), s.run(b, train=train)
        torch.cuda.synchronize()
        assert _bits(ta[0], tb[0]) and _bits(ta[1], tb[1])
        assert _bits(a.rewards, b.rewards) and _bits(a.final, b.final) and _bits(a.z1, b.z1)
    assert _bits(a.grad, b.grad) and bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().sum()) > 0
    for m in range(K):
        assert not torch.equal(a.grad[m], a.grad[(m + 1) % K])
    # the default route ran the model launches, the other one the single-model kernels of the same names
    assert a._models_ok and a.last_kernels["z1"].endswith(",models=3>")
    for i in range(3):
        wa, wb, ra, rb = (e.last_kernels[k % i] for k in ("wgrad%d", "reduce%d") for e in (a, b))
        assert wa.endswith(",models=3>") and wa.replace(",models=3", "") == wb, (wa, wb)
        assert ra.endswith(",models=3") and ra.replace(",models=3", "") == rb, (ra, rb)
    assert a.last_kernels["z1"].replace(",models=3", "") == b.last_kernels["z1"]


# ---- binding -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", base.ENGINE_CASES)
def test_bound_parameters_are_views_of_the_packed_rows(name):
    s = _setting(name)
    ens = s.engine(bound=False)
    before = s.run(ens)
    grad_before, rewards_before = ens.grad.clone(), ens.rewards.clone()
    single_before = [FusedRollout(m, s.c["problem_params"], DEV).run(s.data, s.T, s.ignore, train=False, observation_params=s.obs)
                     for m in ens.models]
    ens.bind_parameters()   # (the first layers are materialised: binds at once)
    assert ens._bound and ens.param_shapes == [tuple(p_.shape) for lin in ens.models[0].master_linears() for p_ in (lin.weight, lin.bias)]
    lo, P = ens.weights.data_ptr(), ens.weights.shape[1]
    for m, model in enumerate(ens.models):
        for p_ in model.parameters():
            assert lo + 4 * m * P <= p_.data_ptr() < lo + 4 * (m + 1) * P
    assert _bits(ens.weights, _packed(ens.models))
    after = s.run(ens)
    torch.cuda.synchronize()
    assert _bits(after[0], before[0]) and _bits(after[1], before[1]) and _bits(ens.grad, grad_before) and _bits(ens.rewards, rewards_before)
    for m, model in enumerate(ens.models):   # a single-model engine on a bound model: the same costs as before binding
        tot, rep = FusedRollout(model, s.c["problem_params"], DEV).run(s.data, s.T, s.ignore, train=False, observation_params=s.obs)
        assert float(tot) == float(single_before[m][0]) and float(rep) == float(single_before[m][1])
    # load_state_dict writes the packed row
    sd = copy.deepcopy(ens.models[0].state_dict())
    row1 = ens.weights[1].clone()
    ens.models[1].load_state_dict(sd)
    assert not torch.equal(ens.weights[1], row1) and _bits(ens.weights[1], ens.weights[0])
    swapped = s.run(ens, train=False)
    assert float(swapped[0][1]) == float(swapped[0][0]) != float(swapped[0][2])


# ---- the step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", base.ENGINE_CASES)
def test_train_step_equals_run_then_step_on_a_twin(name):
    s = _setting(name)
    ours, twin = s.engine(), s.engine()
    opt, opt_twin = s.optimizer(ours), s.optimizer(twin)
    start = ours.weights.clone()
    assert _bits(start, twin.weights)
    for _ in range(3):
        got = s.step(ours, opt)
        want = s.run(twin)
        opt_twin.step(twin.weights, twin.grad)
        assert _bits(got[0], want[0]) and _bits(got[1], want[1])
    torch.cuda.synchronize()
    assert _bits(ours.weights, twin.weights) and _bits(ours.grad, twin.grad)
    assert _bits(opt.exp_avg, opt_twin.exp_avg) and _bits(opt.exp_avg_sq, opt_twin.exp_avg_sq) and _bits(opt.state, opt_twin.state)
    assert opt.steps().tolist() == [3, 3, 3]
    assert bool(torch.isfinite(ours.weights).all())
    for m in range(K):
        assert not torch.equal(ours.weights[m], start[m])
    assert all(p_.grad is None for m in ours.models for p_ in m.parameters())   # train_step assigns no param.grad


def test_three_steps_against_fused_rollout_and_torch_adam():
    """The same three steps by K x (FusedRollout.run + torch.optim.Adam), every one of them held to the referee bar: step i starts
    both sides from OUR parameters and moments after i steps (torch's side on a twin loaded from that state, as
    test_gpu_ensemble_adam.test_a_checkpointed_run_equals_an_uninterrupted_one does), so the gradients are the same bits and the
    float64 Adam from that state referees the two updates."""
    s = _setting(base.ENGINE_CASES[0])
    ours = s.engine()
    opt = s.optimizer(ours)
    hyper = np.array([[lr, 0.9, 0.999, 1e-8, 0.0] for lr in LRS])
    theirs = base._models(s.g, s.g.fresh_config())
    engines = [FusedRollout(m, s.c["problem_params"], DEV) for m in theirs]
    for i in range(3):
        params_i, m_i, v_i = ours.weights.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
        opts = []
        for m, (mine, twin) in enumerate(zip(ours.models, theirs)):
            twin.load_state_dict(mine.state_dict())
            opts.append(torch.optim.Adam(twin.parameters(), lr=LRS[m]))
            if i > 0:
                opts[-1].load_state_dict(copy.deepcopy(opt.state_dict(m)))
        assert _bits(params_i, _packed(theirs))
        s.step(ours, opt)
        for eng, o in zip(engines, opts):
            eng.run(s.data, s.T, s.ignore, observation_params=s.obs)
            assert eng.horizon is not None
        grads = torch.stack([torch.cat([p_.grad.reshape(-1) for lin in m.master_linears() for p_ in (lin.weight, lin.bias)]) for m in theirs])
        assert _bits(ours.grad, grads), i
        for o in opts:
            o.step()
        _referee(params_i, ours.grad, hyper, ours.weights, _packed(theirs), "step %d" % (i + 1), m_i, v_i, i)
    assert opt.steps().tolist() == [3, 3, 3] and bool(torch.isfinite(ours.weights).all())


def test_steps_over_changing_shapes_and_an_evaluation_in_between():
    s = _setting(base.ENGINE_CASES[0])
    half = {k: v[:5].contiguous() for k, v in s.data.items()}   # another batch size (B = 5)
    plan = [(s.data, s.T), (half, s.T), (s.data, s.T - 3), (s.data, s.T)]
    ours, twin = s.engine(), s.engine(model_gemms=False)
    opt, opt_twin = s.optimizer(ours), s.optimizer(twin)
    for i, (data, T) in enumerate(plan):
        got = s.step(ours, opt, data, T)
        want = s.run(twin, data, T)
        opt_twin.step(twin.weights, twin.grad)
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), i
        if i == 1:   # an evaluation between two steps: the optimizer state and the parameters stay
            snap = [t.clone() for t in (opt.exp_avg, opt.exp_avg_sq, opt.state, ours.weights)]
            ev = s.run(ours, train=False)
            ev_twin = s.run(twin, train=False)
            assert _bits(ev[0], ev_twin[0]) and _bits(ev[1], ev_twin[1])
            assert all(_bits(a, b) for a, b in zip(snap, (opt.exp_avg, opt.exp_avg_sq, opt.state, ours.weights)))
    torch.cuda.synchronize()
    assert _bits(ours.weights, twin.weights) and _bits(opt.exp_avg, opt_twin.exp_avg) and _bits(opt.exp_avg_sq, opt_twin.exp_avg_sq)
    assert opt.steps().tolist() == [4, 4, 4]


# ---- fit -----------------------------------------------------------------------------------------------------------------------------
def test_fit_equals_its_hand_written_loop():
    s = _setting(base.ENGINE_CASES[0])
    B = s.data["demands"].shape[0]
    halves = [{k: v[:B // 2].contiguous() for k, v in s.data.items()}, {k: v[B // 2:].contiguous() for k, v in s.data.items()}]
    dev_batches, epochs, n_stores = [s.data], 2, s.c["problem_params"]["n_stores"]
    ours, hand = s.engine(), s.engine()
    opt, opt_hand = s.optimizer(ours), s.optimizer(hand)
    train_hist, dev_hist = ours.fit(halves, dev_batches, epochs, s.T, s.T, s.ignore, opt, s.obs)
    assert train_hist.shape == dev_hist.shape == (epochs, K)
    want_train, want_dev, snapshots = torch.zeros(epochs, K, device=DEV), torch.zeros(epochs, K, device=DEV), []
    for e in range(epochs):
        for data in halves:
            want_train[e] += s.step(hand, opt_hand, data)[1]
        want_train[e] /= float(B * (s.T - s.ignore) * n_stores)
        for data in dev_batches:
            want_dev[e] += s.run(hand, data, train=False)[1]
        want_dev[e] /= float(B * (s.T - s.ignore) * n_stores)
        snapshots.append(hand.weights.clone())
    torch.cuda.synchronize()
    assert _bits(train_hist, want_train) and _bits(dev_hist, want_dev) and _bits(ours.weights, hand.weights)
    # best_dev / best_weights against a host recomputation (the first epoch with the lowest dev loss)
    best = dev_hist.cpu().argmin(dim=0).tolist()
    assert torch.equal(ours.best_dev.cpu(), dev_hist.cpu().min(dim=0).values)
    for m in range(K):
        assert _bits(ours.best_weights[m], snapshots[best[m]][m]), m
    ours.weights.add_(1.0)
    ours.load_best()
    assert _bits(ours.weights, ours.best_weights) and _bits(_packed(ours.models), ours.best_weights)
    assert opt.steps().tolist() == [2 * epochs] * K


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_step():
    s = _setting(base.ENGINE_CASES[0])
    ens = s.engine(bound=False)
    with pytest.raises(ValueError, match="needs bound parameters"):
        s.step(ens, EnsembleAdam(K, 10, DEV, lr=1e-3))
    ens.bind_parameters()
    P = ens.weights.shape[1]
    before = ens.weights.clone()
    for bad in (EnsembleAdam(K, P + 1, DEV, lr=1e-3), EnsembleAdam(K - 1, P, DEV, lr=1e-3)):
        with pytest.raises(ValueError, match=r"the optimizer is for \d+ models of \d+ parameters, the engine has 3 of %d" % P):
            s.step(ens, bad)
    with pytest.raises(ValueError, match="needs an EnsembleAdam"):
        s.step(ens, torch.optim.Adam(ens.models[0].parameters()))
    with pytest.raises(ValueError, match="evaluation-time option"):   # rounded orders have no gradient: no training step takes them
        s.run(ens, train=True, discrete_allocation=True)
    with pytest.raises(TypeError):
        ens.train_step(s.data, s.T, s.ignore, s.optimizer(ens), s.obs, discrete_allocation=True)
    torch.cuda.synchronize()
    assert _bits(ens.weights, before)
    assert sum(n * k + n for _, n, k, _ in layer_slices(ens.dims)) == P
    with pytest.raises(ValueError, match="load_best: no fit"):
        ens.load_best()
