"""Per-model early stopping in the K-model sweeps on a real MI355X: the active-model mask of the `_active` entry points
(nic_small_rollout_ensemble_* / _instances_* / nic_ensemble_adam_*), `EnsembleStep.set_active` and `fit(trainer_params=...)`.

The contract: for a model whose mask entry is zero NO launch reads or writes a byte of its slices - every per-model buffer is
pre-filled with a sentinel bit pattern and must hold it afterwards over the whole slice, padding included; for a model that runs,
every output is the bits of the entry point without the mask on the same inputs.  Shapes are the smallest at which the kernels
can go wrong: 48 scenarios (three 16-lane wavefronts, one and a half 32-lane ones), 6 periods, K = 3 on one batch and K = 4 as 2
instances x 2 replicas, both heads at the depths compiled in for them, both lane widths."""
import functools

import pytest
import torch

import test_gpu_horizon_ensemble_step as hz_step
from neural_inventory_control_amd import _lib, small_rollout as sr
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam
from neural_inventory_control_amd.layout import EnvProblem, Table
from neural_inventory_control_amd.small_ensemble import SmallPolicyEnsemble
from test_gpu_small_ensemble import DEV, PAD, ROW_PAD, _clones, _fresh_models, _random_packed, _Setting, _workload
from test_gpu_small_instances import _instance_data, _Instances

pytestmark = pytest.mark.gpu
B, T, IGN = 48, 6, 2
SENTINEL_BITS = 0x7FA5C3E1   # (a NaN with a payload no kernel produces)
HEADS = {"one_store": ("cfg1", 3), "serial": ("cfg4", 2)}   # vanilla_one_store on one-store lost demand, vanilla_serial on the serial system


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                     b.reshape(-1).contiguous().view(torch.uint8))


def _sentinel(*shape):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL_BITS).all())


def _mask_tensor(mask):
    return None if mask is None else torch.tensor(mask, dtype=torch.int32, device=DEV)


# ---- launch level, through the C ABI ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _settings(head, I):
    """I problem instances (I = 1: the batch itself) of the head's workload at (B, T) as launch-level settings"""
    workload, n_hidden = HEADS[head]
    setting, _, _, _, data = _workload(workload, B, T)
    out = []
    for i in range(I):
        d = data if I == 1 else _instance_data(data, i, False)
        prob = EnvProblem(setting["problem_params"], d, DEV)
        if head == "one_store":
            kind, F, n_out = "softplus", prob.Ws, 1
            assert prob.lost_demand
        else:
            kind, F, n_out = "serial", prob.Ws + prob.Ww + prob.E * prob.We, prob.E + 2
        dims = [F] + [32] * n_hidden + [n_out]
        assert sr.SmallRolloutPlan.supports(prob, kind, dims)
        out.append(_Setting(prob, kind, dims, d, T, 37.0, setting["problem_params"]["n_stores"]))
    return out


KEYS = ("rewards", "final_state", "states", "hidden", "logits", "slab", "grad", "scratch")


def _launch(settings, packed, width, masked, mask, live):
    """forward, backward and the training reduction on K models through the C ABI, every stride longer than its slice and every
    per-model buffer pre-filled with the sentinel (the live models' cost slices with zeros, as every caller does: the reduction sums
    their padding columns).  masked: through the `_active` entry points with `mask` (a device tensor or None = NULL), else the
    entry points without a mask.  len(settings) > 1: the instances entry points.  Returns the buffers and the recorded names."""
    s, K = settings[0], packed.shape[0]
    ins = _Instances(settings) if len(settings) > 1 else None
    w = _sentinel(K, s.P0 + PAD["weights"])
    w[:, :s.P0] = packed
    w_before = w.clone()
    d = s.desc(w, width)
    if ins is not None:
        d = ins.point(d)
    sl = sr.ensemble_slices(d)
    st = {k: sl[k] + PAD[k] for k in ("weights", "rewards", "final_state", "states", "hidden", "logits")}
    row = s.P0 + ROW_PAD
    st["slab"] = sl["slab_rows"] * row + PAD["slab"]
    st["grad"] = s.P0 + PAD["grad"]
    st["scratch"] = sr.small_rollout_reduce_scratch(sl["slab_rows"], s.P0, sl["rewards"]) + PAD["scratch"]
    ens = sr.ensemble_strides(K, **st)
    buf = {k: _sentinel(K, st[k]) for k in KEYS}
    buf["totals"] = _sentinel(K, 2)
    for m in range(K):
        if live[m]:
            buf["rewards"][m, :sl["rewards"]] = 0.0
    lib, stream = _lib.lib(), _lib.current_stream()
    p = {k: t.data_ptr() for k, t in buf.items()}
    hist = (p["states"], p["hidden"], p["logits"])
    where = (d, ens) if ins is None else (d, ens, ins.inst)
    kind = "ensemble" if ins is None else "instances"
    tail = ((None if mask is None else mask.data_ptr()), stream) if masked else (stream,)
    suffix = "_active" if masked else ""
    names = {}
    _lib.check(getattr(lib, f"nic_small_rollout_{kind}_fwd{suffix}")(*where, p["rewards"], p["final_state"], *hist, *tail))
    names["fwd"] = lib.nic_last_kernel().decode()
    _lib.check(getattr(lib, f"nic_small_rollout_{kind}_bwd_wgrad{suffix}")(*where, *hist, Table(s.g_reward, 0, 1).t2(), p["slab"], row, *tail))
    names["bwd"] = lib.nic_last_kernel().decode()
    _lib.check(getattr(lib, f"nic_small_rollout_ensemble_reduce{suffix}")(ens, p["slab"], sl["slab_rows"], row, s.P0, p["grad"], p["rewards"],
                                                                          sl["rewards"], IGN * s.prob.ldb, p["totals"], p["scratch"], *tail))
    names["reduce"] = lib.nic_last_kernel().decode()
    torch.cuda.synchronize()
    buf["weights"] = w
    return buf, names, w_before


# (K, instances, the masks; None: a NULL mask)
CASES = {"one_batch": (3, 1, ([1, 0, 1], [0, 0, 1], [1, 1, 1], None)), "instances": (4, 2, ([1, 0, 0, 1], [1, 1, 1, 1], None))}


@pytest.mark.parametrize("width", [16, 32])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("head", sorted(HEADS))
def test_masked_launches_leave_inactive_slices_alone_and_give_active_ones_the_unmasked_bits(head, case, width):
    K, I, masks = CASES[case]
    settings = _settings(head, I)
    packed = _random_packed(settings[0], K, 7 + K)
    ref, ref_names, _ = _launch(settings, packed, width, False, None, [1] * K)   # the entry points as they are, once for all masks
    assert all(f"models={K}" in n and "active" not in n for n in ref_names.values())
    assert bool(torch.isfinite(ref["totals"]).all()) and bool(torch.isfinite(ref["grad"][:, :settings[0].P0]).all())
    assert not _bits(ref["totals"][0], ref["totals"][K - 1])
    for mask in masks:
        live = [1] * K if mask is None else mask
        got, names, w_in = _launch(settings, packed, width, True, _mask_tensor(mask), live)
        for tag, name in names.items():
            assert name == ref_names[tag][:-1] + ",active>", (tag, name)
        assert _bits(got["weights"], w_in)   # (read only)
        for m in range(K):
            for k in KEYS + ("totals",):
                if live[m]:
                    assert _bits(got[k][m], ref[k][m]), (mask, k, m)       # the whole row: slice and padding
                else:
                    assert _is_sentinel(got[k][m]), (mask, k, m)            # not a byte of it written
    # (that the inactive slices were not READ either: they held NaN patterns and every active result above is the reference's)


def test_a_refused_mask_launches_nothing():
    settings = _settings("one_store", 1)
    s, K = settings[0], 3
    w = _random_packed(s, K, 3)
    d = s.desc(w, 16)
    sl = sr.ensemble_slices(d)
    ens = sr.ensemble_strides(K, **{k: sl[k] for k in ("weights", "rewards", "final_state")})
    out = {k: _sentinel(K, sl[k]) for k in ("rewards", "final_state")}
    mask = torch.ones(K + 1, dtype=torch.int32, device=DEV)
    lib = _lib.lib()
    assert lib.nic_small_rollout_ensemble_fwd_active(d, ens, out["rewards"].data_ptr(), out["final_state"].data_ptr(), None, None, None,
                                                     mask.data_ptr() + 2, _lib.current_stream()) != 0
    message = lib.nic_last_error().decode()
    assert message.startswith("nic_small_rollout_ensemble_fwd_active:") and "4-byte aligned" in message, message
    torch.cuda.synchronize()
    assert all(_is_sentinel(t) for t in out.values())


# ---- the optimizer ---------------------------------------------------------------------------------------------------------------------
K_OPT, P_OPT, P_PAD = 3, 300, 4   # (two column blocks of 256, the second ragged; rows longer than P)
OPT_FIELDS = ("exp_avg", "exp_avg_sq", "state", "coef")


def _optimizer(clipped):
    return EnsembleAdam(K_OPT, P_OPT, DEV, lr=[1e-2, 3e-2, 1e-3], weight_decay=[0.0, 0.01, 0.0],
                        max_grad_norm=[0.5, 1.0, None] if clipped else None)


def _opt_inputs(steps=3):
    gen = torch.Generator().manual_seed(5)
    params = _sentinel(K_OPT, P_OPT + P_PAD)
    params[:, :P_OPT] = torch.randn(K_OPT, P_OPT, generator=gen).to(DEV)
    grads = [torch.randn(K_OPT, P_OPT + P_PAD, generator=gen).to(DEV) for _ in range(steps)]
    return params, grads


def _opt_fields(opt):
    return OPT_FIELDS + (("clip",) if opt.clip is not None else ())


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 0, 1], [1, 1, 1]])
def test_masked_adam_freezes_inactive_rows_and_steps_active_ones_as_unmasked(clipped, mask):
    params0, grads = _opt_inputs()
    ours, ref = _optimizer(clipped), _optimizer(clipped)
    p_ours, p_ref = params0.clone(), params0.clone()
    start = {f: getattr(ours, f).clone() for f in _opt_fields(ours)}
    active = _mask_tensor(mask)
    for g in grads:
        ours.step(p_ours, g, active=active)
        ref.step(p_ref, g)
    torch.cuda.synchronize()
    assert ours.last_kernels["update"].endswith(",active>") and ours.last_kernels["prepare"].endswith(",active>")
    assert ("clipped" in ours.last_kernels["prepare"]) == clipped and not ref.last_kernels["update"].endswith(",active>")
    for m in range(K_OPT):
        if mask[m]:
            assert _bits(p_ours[m], p_ref[m]), m
            for f in _opt_fields(ours):
                assert _bits(getattr(ours, f)[m], getattr(ref, f)[m]), (f, m)
        else:
            assert _bits(p_ours[m], params0[m]), m
            for f in _opt_fields(ours):
                assert _bits(getattr(ours, f)[m], start[f][m]), (f, m)
    assert ours.steps().tolist() == [3 * v for v in mask]
    assert _is_sentinel(p_ours[:, P_OPT:])   # columns at or past P: never written


@pytest.mark.parametrize("clipped", [False, True])
def test_a_model_that_sits_one_step_out_has_taken_two(clipped):
    params0, grads = _opt_inputs()
    ours, two = _optimizer(clipped), _optimizer(clipped)
    p_ours, p_two = params0.clone(), params0.clone()
    for g, mask in zip(grads, ([1, 1, 1], [1, 0, 1], [1, 1, 1])):
        ours.step(p_ours, g, active=_mask_tensor(mask))
    for g in (grads[0], grads[2]):   # model 1's two steps, unmasked
        two.step(p_two, g)
    torch.cuda.synchronize()
    assert ours.steps().tolist() == [3, 2, 3] and two.steps().tolist() == [2, 2, 2]
    assert _bits(ours.state[1], two.state[1])   # the counter and the running products c1, c2
    assert _bits(p_ours[1], p_two[1]) and _bits(ours.exp_avg[1], two.exp_avg[1]) and _bits(ours.exp_avg_sq[1], two.exp_avg_sq[1])
    assert _bits(ours.coef[1], two.coef[1])
    assert not _bits(p_ours[0], p_two[0])       # (a model that took all three is somewhere else)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def _adam(ens, lrs):
    return EnsembleAdam(ens.n_models, ens.weights.shape[1], DEV, lr=list(lrs), param_shapes=ens.param_shapes)


@functools.lru_cache(maxsize=None)
def _batches(n, I):
    """n batches of the cfg1 pool: dicts (I = 1) or lists of I instances' dicts with scaled underage costs"""
    setting, _, obs, _, pool = _workload("cfg1", n * I * B, T)
    out = []
    for j in range(n):
        row = []
        for i in range(I):
            data = {k: v[(j * I + i) * B:(j * I + i + 1) * B] for k, v in pool.items()}
            row.append(dict(data, underage_costs=data["underage_costs"] * (1.0 + 1.25 * i)))
        out.append(row[0] if I == 1 else row)
    return setting, obs, out


def _engine(models, setting, use_graph, lrs):
    ens = SmallPolicyEnsemble(models, setting["problem_params"], DEV)
    ens.use_graph = use_graph
    ens.bind_parameters()
    return ens, _adam(ens, lrs)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("I", [1, 2])
def test_engine_steps_follow_the_mask_between_replays(I, use_graph):
    K = 3 if I == 1 else 4
    masks = ([1, 0, 1], [1, 1, 0]) if I == 1 else ([1, 0, 0, 1], [1, 1, 0, 1])
    setting, obs, batches = _batches(5, I)
    lrs = (1e-2, 3e-3, 1e-3, 3e-2)[:K]
    models = _fresh_models("cfg1", 5 * I * B, T, tuple(range(71, 71 + K)))
    ours, opt = _engine(models, setting, use_graph, lrs)
    twin, topt = _engine(_clones(models), setting, False, lrs)   # never masked: what an active model's step must give
    assert ours.active.dtype == torch.int32 and ours.active_models().tolist() == [True] * K
    address = ours.active.data_ptr()
    # until a mask is set: the launches as they always were
    got, want = ours.train_step(batches[0], T, IGN, opt, obs), twin.train_step(batches[0], T, IGN, topt, obs)
    assert _bits(got[0], want[0]) and _bits(ours.weights, twin.weights)
    assert not any("active" in n for n in ours.last_kernels.values()) and not opt.last_kernels["update"].endswith(",active>")
    graphs = None
    always = [m for m in range(K) if all(mask[m] for mask in masks)]
    for step, mask in ((1, masks[0]), (2, masks[0]), (3, masks[1]), (4, masks[1])):
        ours.set_active(mask)
        assert ours.active.data_ptr() == address and ours.active_models().tolist() == [bool(v) for v in mask]
        before = ours.weights.clone()
        total, reported = ours.train_step(batches[step], T, IGN, opt, obs)
        want = twin.train_step(batches[step], T, IGN, topt, obs)
        torch.cuda.synchronize()
        assert all(ours.last_kernels[k].endswith(",active>") for k in ("fwd", "bwd", "reduce")), ours.last_kernels
        assert opt.last_kernels["prepare"].endswith(",active>") and opt.last_kernels["update"].endswith(",active>")
        assert torch.isnan(total).tolist() == torch.isnan(reported).tolist() == [not v for v in mask]   # NaN exactly on the inactive models
        for m in range(K):
            if not mask[m]:
                assert _bits(ours.weights[m], before[m]), (step, m)
        for m in always:   # active all along: the bits of an engine that never had a mask
            assert _bits(total[m], want[0][m]) and _bits(reported[m], want[1][m]) and _bits(ours.weights[m], twin.weights[m]), (step, m)
        if use_graph:
            if step == 2:
                graphs = len(ours._graphs)
                assert graphs >= 1
            elif step > 2:
                assert len(ours._graphs) == graphs   # another mask, the same batch shape: no new capture
    assert opt.steps().tolist() == [1 + 2 * masks[0][m] + 2 * masks[1][m] for m in range(K)]
    # an evaluation under the mask, then every model again through the launches without one
    total, _ = ours.run(batches[0], T, IGN, train=False, observation_params=obs)
    assert torch.isnan(total).tolist() == [not v for v in masks[1]] and ours.last_kernels["fwd"].endswith(",active>")
    ours.set_active(None)
    total, _ = ours.run(batches[0], T, IGN, train=False, observation_params=obs)
    assert bool(torch.isfinite(total).all()) and "active" not in ours.last_kernels["fwd"] and ours.active_models().tolist() == [True] * K


def test_horizon_ensemble_freezes_a_stopped_models_row():
    s = hz_step._setting(hz_step.base.ENGINE_CASES[0])
    ens = s.engine()
    opt = s.optimizer(ens)
    s.step(ens, opt)
    ens.set_active([1, 0, 1])
    frozen, moments, state = ens.weights[1].clone(), opt.exp_avg[1].clone(), opt.state[1].clone()
    moving = ens.weights[0].clone()
    for _ in range(2):
        total, _ = s.step(ens, opt)
    torch.cuda.synchronize()
    assert _bits(ens.weights[1], frozen) and _bits(opt.exp_avg[1], moments) and _bits(opt.state[1], state)
    assert not _bits(ens.weights[0], moving) and opt.steps().tolist() == [3, 1, 3]
    assert bool(torch.isfinite(total).all())   # (its launches still run every model: the costs are computed)


# ---- fit with early stopping -----------------------------------------------------------------------------------------------------------
FIT_LRS = (1e-3, 1e3, 3e-2)   # a small step, an absurd one (its loss never improves on the first epoch's), one in between
TRAINER = {"do_dev_every_n_epochs": 1, "choose_best_model_on": "dev_loss", "early_stopping_patience_epochs": 2,
           "save_model": False, "print_results_every_n_epochs": 1}
EPOCHS = 8


def _fit_models(K):
    one = _fresh_models("cfg1", 3 * B, T, (91,))[0]
    return [_clones([one])[0] for _ in range(K)]   # the same initial weights, K separate models


@pytest.mark.parametrize("use_graph", [False, True])
def test_fit_with_early_stopping_equals_one_model_ensembles_running_the_same_fit(use_graph):
    K = len(FIT_LRS)
    setting, obs, batches = _batches(3, 1)
    train, dev = batches[:2], batches[2:]
    ens, opt = _engine(_fit_models(K), setting, use_graph, FIT_LRS)
    train_hist, dev_hist = ens.fit(train, dev, EPOCHS, T, T, IGN, opt, obs, trainer_params=TRAINER)
    torch.cuda.synchronize()
    stopped = ens.stopped_epoch.tolist()
    assert len(set(stopped)) >= 2 and min(s for s in stopped if s >= 0) < EPOCHS - 1, stopped   # they stop at different epochs
    for m in range(K):
        alone, aopt = _engine(_fit_models(1), setting, use_graph, FIT_LRS[m:m + 1])
        th, dh = alone.fit(train, dev, EPOCHS, T, T, IGN, aopt, obs, trainer_params=TRAINER)
        torch.cuda.synchronize()
        assert int(ens.stopped_epoch[m]) == int(alone.stopped_epoch[0]), m
        assert int(ens.best_epoch[m]) == int(alone.best_epoch[0]), m
        assert _bits(ens.best_dev[m], alone.best_dev[0]) and _bits(ens.best_train[m], alone.best_train[0]), m
        assert _bits(ens.best_weights[m], alone.best_weights[0]), m
        assert _bits(ens.weights[m], alone.weights[0]), m           # the final weights: frozen from the stop on
        assert _bits(train_hist[:, m], th[:, 0]) and _bits(dev_hist[:, m], dh[:, 0]), m
        last = stopped[m] if stopped[m] >= 0 else EPOCHS - 1
        assert bool(torch.isfinite(dev_hist[:last + 1, m]).all() or FIT_LRS[m] > 1) and bool(torch.isnan(train_hist[last + 1:, m]).all())
        assert int(opt.steps()[m]) == 2 * (last + 1)                  # two batches an epoch, none after the stop
    assert ens.active_models().tolist() == [s < 0 for s in stopped]
    ens.load_best()
    assert _bits(ens.weights, ens.best_weights)


def test_fit_without_trainer_params_is_the_loop_it_always_was():
    K = 3
    setting, obs, batches = _batches(3, 1)
    train, dev, epochs = batches[:2], batches[2:], 3
    lrs = (1e-2, 3e-3, 1e-3)
    ens, opt = _engine(_fit_models(K), setting, False, lrs)
    train_hist, dev_hist = ens.fit(train, dev, epochs, T, T, IGN, opt, obs, trainer_params=None)
    hand, hopt = _engine(_fit_models(K), setting, False, lrs)
    n_stores = setting["problem_params"]["n_stores"]
    want = [torch.zeros(epochs, K, device=DEV), torch.zeros(epochs, K, device=DEV)]
    best_dev, best_weights = torch.full((K,), float("inf"), device=DEV), None
    for e in range(epochs):
        for data in train:
            want[0][e] += hand.train_step(data, T, IGN, hopt, obs)[1]
        want[0][e] /= float(2 * B * (T - IGN) * n_stores)
        for data in dev:
            want[1][e] += hand.run(data, T, IGN, train=False, observation_params=obs)[1]
        want[1][e] /= float(B * (T - IGN) * n_stores)
        best_weights = hand.weights.clone() if best_weights is None else best_weights
        better = want[1][e] < best_dev
        best_dev = torch.where(better, want[1][e], best_dev)
        best_weights = torch.where(better[:, None], hand.weights, best_weights)
    torch.cuda.synchronize()
    assert _bits(train_hist, want[0]) and _bits(dev_hist, want[1]) and _bits(ens.weights, hand.weights)
    assert _bits(ens.best_dev, best_dev) and _bits(ens.best_weights, best_weights)
    assert ens.stopped_epoch is None and ens.active_models().tolist() == [True] * K
    assert not any("active" in n for n in ens.last_kernels.values())
