"""The fused Adam of K small policies and the replayed training step (nic_ensemble_adam_*, EnsembleAdam,
SmallPolicyEnsemble.bind_parameters / train_step / fit) on a real MI355X.

Kernel level the bar is BIT equality with the host build of csrc/ensemble_adam_body.h (tests/ensemble_adam_harness.cpp), with every
stride longer than P and NaN in every gap; engine level it is bit equality between the routes that must run the same arithmetic
(train_step against run + step on an unbound twin, replayed against eager, a checkpointed run against an uninterrupted one, fit
against its hand-written loop) and, against torch.optim.Adam, the self-measuring referee bar of test_ensemble_adam_host.py: our
error against a float64 Adam on the same gradients is at most 2 x torch's own."""
import copy
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

import ensemble_adam_checks as eac
from neural_inventory_control_amd import _lib, ensemble_step as es, small_rollout as sr, workloads
from neural_inventory_control_amd.data_handling import Scenario
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
from neural_inventory_control_amd.neural_networks import NeuralNetworkCreator
from neural_inventory_control_amd.policy_layers import materialize_linears
from neural_inventory_control_amd.rollout import FusedRollout
from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PADS = (3, 5, 1, 2)   # floats past P in a row of params / grads / exp_avg / exp_avg_sq


def _bits(a, b):
    """bit equality (NaN-filled regions that nobody wrote compare equal too)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("ensemble_adam_gpu")
    return eac.build_harness(d), d


# ---- kernel level --------------------------------------------------------------------------------------------------------------------
def _padded_inputs(P, rows):
    """the host test's inputs for P, models `rows`, every stride P + another pad with NaN in the gap"""
    params, grads, hyper = eac.inputs(P)
    params, grads, hyper = params[rows], grads[:, rows], hyper[rows]
    zeros = np.zeros_like(params)
    return (eac.padded(params, P + PADS[0]), eac.padded(grads, P + PADS[1]), hyper, eac.padded(zeros, P + PADS[2]),
            eac.padded(zeros, P + PADS[3]), eac.fresh_state(len(rows)))


def _device_steps(P, params, grads, hyper, exp_avg, exp_avg_sq, state):
    K, lib, stream = params.shape[0], _lib.lib(), _lib.current_stream()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in dict(params=params, grads=grads, hyper=hyper, exp_avg=exp_avg,
                                                                                 exp_avg_sq=exp_avg_sq).items()}
    t["state"] = torch.from_numpy(np.frombuffer(state.tobytes(), dtype=np.float64).reshape(K, 3).copy()).to(DEV)
    t["coef"] = torch.zeros(K, eac.N_COEF, device=DEV)
    names = set()
    for s in range(grads.shape[0]):
        _lib.check(lib.nic_ensemble_adam_prepare(K, t["hyper"].data_ptr(), t["state"].data_ptr(), t["coef"].data_ptr(), stream))
        names.add(lib.nic_last_kernel().decode())
        _lib.check(lib.nic_ensemble_adam_update(K, P, t["params"].data_ptr(), params.shape[1], t["grads"][s].data_ptr(), grads.shape[2],
                                                t["exp_avg"].data_ptr(), exp_avg.shape[1], t["exp_avg_sq"].data_ptr(), exp_avg_sq.shape[1],
                                                t["coef"].data_ptr(), stream))
        names.add(lib.nic_last_kernel().decode())
    torch.cuda.synchronize()
    assert names == {f"ensemble_adam_prepare<models={K}>", f"ensemble_adam_update<{P},models={K}>"}
    out = {k: t[k].cpu().numpy() for k in ("params", "exp_avg", "exp_avg_sq", "coef")}
    out["state"] = np.frombuffer(t["state"].cpu().numpy().tobytes(), dtype=eac.STATE_DTYPE)
    return out


def _same(got, want, P):
    for k in ("params", "exp_avg", "exp_avg_sq", "coef"):
        assert got[k].tobytes() == want[k].tobytes(), k   # (live columns and the NaN of every gap, bit for bit)
    assert got["state"].tobytes() == want["state"].tobytes()
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert np.isfinite(got[k][:, :P]).all() and np.isnan(got[k][:, P:]).all(), k


@pytest.mark.parametrize("P", [1, 255, 256, 257, 2305])
@pytest.mark.parametrize("K", [1, 3])
def test_kernels_equal_the_host_build_of_the_body_bit_for_bit(harness, K, P):
    """relies on -ffp-contract=off, correctly rounded float division and square root, and inputs that produce no denormals"""
    exe, d = harness
    args = _padded_inputs(P, list(range(K)))
    got = _device_steps(P, *args)
    _same(got, eac.run_harness(exe, d, P, *args), P)
    assert list(got["state"]["step"]) == [eac.STEPS] * K


@pytest.mark.parametrize("P", [257, 2305])
def test_a_row_of_three_equals_a_launch_of_one_on_that_row(P):
    three = _device_steps(P, *_padded_inputs(P, [0, 1, 2]))
    for m in range(3):
        one = _device_steps(P, *_padded_inputs(P, [m]))
        for k in ("params", "exp_avg", "exp_avg_sq", "coef", "state"):
            assert three[k][m:m + 1].tobytes() == one[k].tobytes(), (k, m)


@pytest.mark.parametrize("what", ["no_models", "too_many_models", "no_columns", "null_grads", "null_state", "short_params_stride",
                                  "short_grads_stride", "short_exp_avg_stride", "short_exp_avg_sq_stride"])
def test_refused_requests_launch_nothing(what):
    """non-zero status, a message, and the poisoned buffers unchanged"""
    K, P, POISON = 3, 257, -12345.0
    buf = {k: torch.full((K, P), POISON, device=DEV) for k in ("params", "grads", "exp_avg", "exp_avg_sq")}
    hyper = torch.tensor(eac.HYPER, dtype=torch.float64, device=DEV)
    state = torch.full((K, 3), POISON, dtype=torch.float64, device=DEV)
    coef = torch.full((K, eac.N_COEF), POISON, device=DEV)
    n, cols = {"no_models": (0, P), "too_many_models": (65536, P), "no_columns": (K, 0)}.get(what, (K, P))
    stride = {k: P - 1 if what == f"short_{k}_stride" else P for k in buf}
    ptr = {k: None if what == f"null_{k}" else t.data_ptr() for k, t in buf.items()}
    lib, stream = _lib.lib(), _lib.current_stream()
    if what in ("no_models", "too_many_models", "null_state"):
        assert lib.nic_ensemble_adam_prepare(n, hyper.data_ptr(), None if what == "null_state" else state.data_ptr(), coef.data_ptr(), stream) != 0
        assert lib.nic_last_error().decode().startswith("nic_ensemble_adam_prepare:")
    if what != "null_state":
        assert lib.nic_ensemble_adam_update(n, cols, ptr["params"], stride["params"], ptr["grads"], stride["grads"], ptr["exp_avg"],
                                            stride["exp_avg"], ptr["exp_avg_sq"], stride["exp_avg_sq"], coef.data_ptr(), stream) != 0
        assert lib.nic_last_error().decode().startswith("nic_ensemble_adam_update:")
    torch.cuda.synchronize()
    for k, t in dict(buf, state=state, coef=coef).items():
        assert bool((t == POISON).all()), k


# ---- engine level: cfg1 at B = 128, T = 8, three seeds, three learning rates, five batches ---------------------------------------
B, T, IGNORE, SEEDS, LRS = 128, 8, 2, (21, 22, 23), (1e-2, 3e-3, 1e-3)
LRS_LATER = (5e-3, 1e-3, 2e-2)   # what a scheduler sets between steps 3 and 4


@functools.lru_cache(maxsize=None)
def _workload():
    setting, policy, _, _, _ = workloads.get("cfg1")
    obs = defaultdict(lambda: None, setting["observation_params"])
    sc = Scenario(T, setting["problem_params"], setting["store_params"], setting["warehouse_params"], setting["echelon_params"], 5 * B, obs,
                  setting["seeds"])
    return setting, policy, obs, sc, {k: v.to(DEV) for k, v in sc.get_data().items()}


def _batches(sizes=(B,) * 5):
    pool = _workload()[4]
    return [{k: v[i * B:i * B + n] for k, v in pool.items()} for i, n in enumerate(sizes)]


def _fresh_models():
    setting, policy, obs, sc, data = _workload()
    F = data["initial_inventories"].shape[1] * data["initial_inventories"].shape[2]
    models = []
    for seed in SEEDS:
        torch.manual_seed(seed)
        m = NeuralNetworkCreator().create_neural_network(sc, policy, device=DEV)
        materialize_linears(m.master_linears(), F)
        models.append(m)
    return models


def _engine(bound=True, use_graph=False):
    ens = SmallPolicyEnsemble(_fresh_models(), _workload()[0]["problem_params"], DEV)
    ens.use_graph = use_graph
    if bound:
        ens.bind_parameters()
        assert ens._bound and ens.weights is not None   # (materialised models: bound at once)
    return ens


def _optimizer(ens, lrs=LRS):
    P = sum(p.numel() for p in ens.models[0].parameters())
    return EnsembleAdam(len(SEEDS), P, DEV, lr=lrs, param_shapes=ens.param_shapes or [p.shape for p in ens.models[0].parameters()])


def _snapshot(ens, opt, totals):
    torch.cuda.synchronize()
    return dict(weights=ens.weights.clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), state=opt.state.clone(),
                coef=opt.coef.clone(), totals=torch.stack(totals))


def _train(use_graph=False, lr_change=False, sizes=(B,) * 5):
    ens = _engine(use_graph=use_graph)
    opt = _optimizer(ens)
    obs, totals = _workload()[2], []
    for i, data in enumerate(_batches(sizes)):
        if lr_change and i == 3:
            opt.set_lr(LRS_LATER)
        totals.append(torch.stack(ens.train_step(data, T, IGNORE, opt, obs)))
    return ens, opt, _snapshot(ens, opt, totals)


@functools.lru_cache(maxsize=None)
def _eager(lr_change=False, sizes=(B,) * 5):
    """the eager runs the other routes are held to: computed once, read only"""
    return _train(False, lr_change, sizes)[2]


def _assert_same(got, want):
    for k in want:
        assert _bits(got[k], want[k]), k


def _write_back(ens):
    """an unbound engine's packed rows -> its models' parameters (what K optimizers on the parameters would have done)"""
    F, nh, no = ens.plan.F, ens.plan.n_hidden, ens.plan.n_out
    with torch.no_grad():
        for model, (ws, bs) in zip(ens.models, es.grad_views(ens.weights, [F] + [sr.H] * nh + [no])):
            for lin, w, b in zip(model.master_linears(), ws, bs):
                lin.weight.copy_(w)
                lin.bias.copy_(b)


def _packed(models):
    return torch.stack([sr.pack_weights(m.master_linears()) for m in models])


def test_train_step_equals_run_then_step_on_an_unbound_twin():
    want = _eager()
    twin = _engine(bound=False)
    opt, obs, totals = _optimizer(twin), _workload()[2], []
    for data in _batches():
        totals.append(torch.stack(twin.run(data, T, IGNORE, train=True, observation_params=obs)))
        opt.step(twin.weights, twin.grad)
        _write_back(twin)
    _assert_same(_snapshot(twin, opt, totals), want)
    assert opt.steps().tolist() == [5, 5, 5]
    assert not torch.equal(want["weights"][0], want["weights"][1]) and bool(torch.isfinite(want["weights"]).all())
    assert (opt.last_kernels["prepare"], opt.last_kernels["update"]) == ("ensemble_adam_prepare<models=3>", "ensemble_adam_update<2305,models=3>")


def _referee(params0, grads, hyper, ours, theirs, what, m0=None, v0=None, t0=0):
    """ours / theirs [K][P] after one step from params0 on `grads`: both against float64 Adam, ours held to 2 x theirs per model"""
    p64 = eac.adam_f64(params0.cpu().numpy(), grads.cpu().numpy()[None], hyper, None if m0 is None else m0.cpu().numpy(),
                       None if v0 is None else v0.cpu().numpy(), t0)
    for m in range(p64.shape[0]):
        err_ours = float(np.abs(ours[m].double().cpu().numpy() - p64[m]).max())
        err_theirs = float(np.abs(theirs[m].double().cpu().numpy() - p64[m]).max())
        print(f"{what}, model {m}: max |error| against float64 Adam: ours {err_ours:.3e}, torch {err_theirs:.3e}")
        assert err_theirs > 0.0
        assert err_ours <= 2.0 * err_theirs, (what, m, err_ours, err_theirs)


def test_against_three_torch_adams():
    """After the first step (the gradients are the same bits) the parameters meet the referee bar; after five the two trajectories may
    have drifted: the difference is reported, not asserted."""
    theirs = _engine(bound=False)
    opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(theirs.models, LRS)]
    ours = _engine()
    opt, obs = _optimizer(ours), _workload()[2]
    params0 = ours.weights.clone()
    assert torch.equal(params0, _packed(theirs.models))
    P = params0.shape[1]
    for i, data in enumerate(_batches()):
        ours.train_step(data, T, IGNORE, opt, obs)
        theirs.run(data, T, IGNORE, train=True, observation_params=obs)
        if i == 0:
            assert _bits(ours.grad, theirs.grad)
        for o in opts:
            o.step()
        if i == 0:
            _referee(params0, ours.grad[:, :P], np.array([[lr, 0.9, 0.999, 1e-8, 0.0] for lr in LRS]), ours.weights,
                     _packed(theirs.models), "step 1")
    diff = (ours.weights - _packed(theirs.models)).abs().max(dim=1).values.tolist()
    print("after five steps, max |ours - torch| per model (reported, not asserted):", ["%.3e" % d for d in diff])
    assert bool(torch.isfinite(ours.weights).all())


# ---- replay ----------------------------------------------------------------------------------------------------------------------------
def test_replayed_steps_equal_eager_steps():
    ens, opt, got = _train(use_graph=True)
    _assert_same(got, _eager())
    assert len(ens._graphs) > 0 and opt.steps().tolist() == [5, 5, 5]


def test_a_new_learning_rate_reaches_a_replayed_step():
    ens, opt, got = _train(use_graph=True, lr_change=True)
    assert len(ens._graphs) > 0
    _assert_same(got, _eager(lr_change=True))
    assert not _bits(got["weights"], _eager()["weights"])   # (the change did something)


def test_a_short_batch_in_between_keeps_parameters_and_optimizer_state():
    """128, 100, 128, 100, 128 scenarios: 100 leave a ragged last wavefront; each shape keeps its buffers and its capture"""
    sizes = (128, 100, 128, 100, 128)
    ens, opt, got = _train(use_graph=True, sizes=sizes)
    _assert_same(got, _eager(sizes=sizes))
    assert len(ens._graphs) > 0 and len(ens._shapes) == 1 and opt.steps().tolist() == [5, 5, 5]
    assert not _bits(got["weights"], _eager()["weights"])


def test_eager_engine_keeps_bound_weights_across_batch_shapes():
    ens = _engine()
    opt, obs = _optimizer(ens), _workload()[2]
    ptrs = None
    for data in _batches((128, 100, 128)):
        ens.train_step(data, T, IGNORE, opt, obs)
        now = (ens.weights.data_ptr(), ens.grad.data_ptr(), next(ens.models[1].parameters()).data_ptr())
        assert ptrs in (None, now)
        ptrs = now
    assert ens._shapes == {}   # (eager launches keep one shape's buffers)


def test_replayed_fit_keeps_the_training_capture_across_the_dev_passes():
    """fit alternates train_step and run(train=False), here on two shapes (the dev pass has 6 periods): under replay the result is
    the eager one bit for bit, and the training shape's buffers and its capture in the last epoch are the first epoch's objects."""
    batches, obs = _batches(), _workload()[2]
    train, dev, T_dev, epochs = batches[:2], batches[2:3], 6, 3
    eager = _engine()
    want = eager.fit(train, dev, epochs, T, T_dev, IGNORE, _optimizer(eager), obs)
    ens = _engine(use_graph=True)
    opt, got, seen = _optimizer(ens), [], []
    for _ in range(epochs):   # (one epoch a call, to look at the training shape in between)
        got.append(ens.fit(train, dev, 1, T, T_dev, IGNORE, opt, obs))
        (st,) = [st for key, st in ens._shapes.items() if key[1] == T]   # (the dev shape is the current one)
        assert ens._key[1] == T_dev and len(st.replay.graphs) == 1
        seen.append((st, st.replay, tuple(st.replay.graphs.values()), st.replay.demand.data_ptr(), st.replay.prob,
                     tuple(getattr(st, n).data_ptr() for n in ("state0", "rewards", "states", "hidden", "logits", "slab", "scratch"))))
    torch.cuda.synchronize()
    assert _bits(torch.cat([g[0] for g in got]), want[0]) and _bits(torch.cat([g[1] for g in got]), want[1])
    assert _bits(ens.weights, eager.weights) and _bits(ens.best_weights, eager.best_weights) and _bits(ens.best_dev, eager.best_dev)
    first, last = seen[0], seen[-1]
    assert all(a is b for a, b in zip(first[:2], last[:2])) and first[4] is last[4]
    assert len(first[2]) == 1 and first[2][0] is last[2][0] and first[3] == last[3] and first[5] == last[5]
    assert len(ens._graphs) == 1   # (the dev shape's own capture, taken in the second epoch)


# ---- bound parameters ------------------------------------------------------------------------------------------------------------------
def test_bound_parameters_are_the_packed_rows():
    ens, opt, got = _train(sizes=(B, B))
    setting, _, obs, _, _ = _workload()
    base, n_bytes = ens.weights.data_ptr(), ens.weights.numel() * 4
    for m, model in enumerate(ens.models):
        sd = model.state_dict()
        flat = torch.cat([sd[k].reshape(-1) for k in sd])
        assert torch.equal(flat, ens.weights[m]) and not torch.equal(flat, _packed(_fresh_models())[m])   # the updated values
        assert all(base <= p.data_ptr() < base + n_bytes for p in model.parameters())
    data = _batches()[4]
    tot, rep = ens.run(data, T, IGNORE, train=False, observation_params=obs)
    for m, model in enumerate(ens.models):
        t1, r1 = FusedRollout(model, setting["problem_params"], DEV).run(data, T, IGNORE, train=False, observation_params=obs)
        assert torch.equal(tot[m], t1) and torch.equal(rep[m], r1)
    # load_state_dict writes through to the packed row, and only to that row
    other = _fresh_models()[2].state_dict()
    before = ens.weights.clone()
    ens.models[0].load_state_dict(other)
    assert torch.equal(ens.weights[0], torch.cat([other[k].reshape(-1) for k in other])) and torch.equal(ens.weights[1:], before[1:])


def test_train_step_needs_bound_parameters_and_an_ensemble_adam():
    ens = _engine(bound=False)
    obs, data = _workload()[2], _batches()[0]
    with pytest.raises(ValueError, match="bind_parameters"):
        ens.train_step(data, T, IGNORE, _optimizer(ens), obs)
    ens.bind_parameters()
    with pytest.raises(ValueError, match="EnsembleAdam"):
        ens.train_step(data, T, IGNORE, torch.optim.Adam(ens.models[0].parameters()), obs)
    with pytest.raises(ValueError, match="optimizer is for"):
        ens.train_step(data, T, IGNORE, EnsembleAdam(2, 2305, DEV, lr=1e-3), obs)


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------------
def test_a_checkpointed_run_equals_an_uninterrupted_one():
    ens = _engine()
    opt, obs, batches, totals = _optimizer(ens), _workload()[2], _batches(), []
    for data in batches[:3]:
        totals.append(torch.stack(ens.train_step(data, T, IGNORE, opt, obs)))
    sds = [opt.state_dict(m) for m in range(3)]
    params3, m3, v3 = ens.weights.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    fresh = _optimizer(ens, lrs=1.0)   # (every hyper-parameter comes from the checkpoint)
    for m, sd in enumerate(sds):
        fresh.load_state_dict(m, sd)
    # the same checkpoint through three default torch.optim.Adam on a twin with the same parameters
    twin = _engine(bound=False)
    for a, b in zip(twin.models, ens.models):
        a.load_state_dict(b.state_dict())
    opts = [torch.optim.Adam(m.parameters()) for m in twin.models]
    for o, sd in zip(opts, sds):
        o.load_state_dict(copy.deepcopy(sd))
    totals.append(torch.stack(ens.train_step(batches[3], T, IGNORE, fresh, obs)))
    twin.run(batches[3], T, IGNORE, train=True, observation_params=obs)
    assert _bits(ens.grad, twin.grad)
    for o in opts:
        o.step()
    hyper = np.array([[lr, 0.9, 0.999, 1e-8, 0.0] for lr in LRS])
    _referee(params3, ens.grad[:, :params3.shape[1]], hyper, ens.weights, _packed(twin.models), "step 4 from the checkpoint", m3, v3, 3)
    totals.append(torch.stack(ens.train_step(batches[4], T, IGNORE, fresh, obs)))
    _assert_same(_snapshot(ens, fresh, totals), _eager())


# ---- fit -------------------------------------------------------------------------------------------------------------------------------
def test_fit_equals_its_hand_written_loop_and_keeps_the_best_weights():
    batches, obs = _batches(), _workload()[2]
    train, dev, epochs, K = batches[:2], batches[2:3], 3, len(SEEDS)
    ens = _engine()
    train_hist, dev_hist = ens.fit(train, dev, epochs, T, T, IGNORE, _optimizer(ens), obs)
    hand = _engine()
    opt = _optimizer(hand)
    n_stores = _workload()[0]["problem_params"]["n_stores"]
    want_train, want_dev, rows = torch.zeros(epochs, K, device=DEV), torch.zeros(epochs, K, device=DEV), []
    for e in range(epochs):
        for data in train:
            want_train[e] += hand.train_step(data, T, IGNORE, opt, obs)[1]
        want_train[e] /= float(2 * B * (T - IGNORE) * n_stores)
        for data in dev:
            want_dev[e] += hand.run(data, T, IGNORE, train=False, observation_params=obs)[1]
        want_dev[e] /= float(B * (T - IGNORE) * n_stores)
        rows.append(hand.weights.clone())
    torch.cuda.synchronize()
    assert _bits(train_hist, want_train) and _bits(dev_hist, want_dev) and _bits(ens.weights, hand.weights)
    assert tuple(train_hist.shape) == (epochs, K) and bool((train_hist > 0).all())
    best = dev_hist.argmin(dim=0).tolist()   # (the first epoch with the lowest dev loss)
    for m, e in enumerate(best):
        assert _bits(ens.best_weights[m], rows[e][m]) and float(ens.best_dev[m]) == float(dev_hist[e, m])
    ens.load_best()
    assert _bits(ens.weights, ens.best_weights)
    sd = ens.models[1].state_dict()
    assert torch.equal(torch.cat([sd[k].reshape(-1) for k in sd]), ens.best_weights[1])
