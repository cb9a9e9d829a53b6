"""Gradient-norm clipping inside the fused Adam of K models (nic_ensemble_adam_prepare_clipped / _update_clipped,
EnsembleAdam(max_grad_norm=...), EnsembleStep.make_optimizer) on a real MI355X.

Kernel level the bar is BIT equality with the host build of csrc/ensemble_clip_body.h (tests/ensemble_clip_harness.cpp) - parameters,
moments, coefficients, state, the clip table of every step and the untouched NaN of every gap.  Engine level it is bit equality
between the routes that must run the same arithmetic (train_step against run + step on an unbound twin, replayed against eager, a
checkpointed run against an uninterrupted one) and, against per-model `clip_grad_norm_` + torch.optim.Adam, the referee bar of
test_gpu_ensemble_adam.py (`_referee`: our error against clipping and Adam in float64 at most 2 x torch's own), with the norms the
optimizer reports within one float32 ulp of float64.  The workloads, models and batches are test_gpu_ensemble_adam's (cfg1, B = 128,
T = 8, three seeds) and test_gpu_horizon_ensemble_step's (the first real-data fixture, K = 3)."""
import copy
import functools

import numpy as np
import pytest
import torch

import ensemble_adam_checks as eac
import ensemble_clip_checks as ecc
import test_gpu_ensemble_adam as tga
import test_gpu_horizon_ensemble_step as ths
from neural_inventory_control_amd import _lib
from neural_inventory_control_amd.ensemble_adam import EnsembleAdam

pytestmark = pytest.mark.gpu
DEV = tga.DEV
PADS = tga.PADS
INF = float("inf")
SIZES = [1, 255, 256, 257, 511, 513, 2305]   # one column, both sides of one and two lane strides, a ragged multi-stride row
_bits = tga._bits


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("ensemble_clip_gpu")
    return ecc.build_harness(d), d


# ---- kernel level --------------------------------------------------------------------------------------------------------------------
def _padded_inputs(P, rows):
    """test_ensemble_clip_host's cases: ensemble_adam_checks.inputs(P), models `rows` with their max norms, every stride P + another
    pad with NaN in the gap"""
    params, grads, hyper = eac.inputs(P)
    params, grads, hyper = params[rows], grads[:, rows], hyper[rows]
    zeros = np.zeros_like(params)
    return (eac.padded(params, P + PADS[0]), eac.padded(grads, P + PADS[1]), hyper, np.array(ecc.MAX_NORMS)[rows],
            eac.padded(zeros, P + PADS[2]), eac.padded(zeros, P + PADS[3]), eac.fresh_state(len(rows)))


def _device_steps(P, params, grads, hyper, max_norm, exp_avg, exp_avg_sq, state):
    K, steps, lib, stream = params.shape[0], grads.shape[0], _lib.lib(), _lib.current_stream()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in dict(params=params, grads=grads, hyper=hyper, max_norm=max_norm,
                                                                                 exp_avg=exp_avg, exp_avg_sq=exp_avg_sq).items()}
    t["state"] = torch.from_numpy(np.frombuffer(state.tobytes(), dtype=np.float64).reshape(K, 3).copy()).to(DEV)
    t["coef"] = torch.zeros(K, eac.N_COEF, device=DEV)
    t["clip"] = torch.zeros(steps, K, ecc.N_CLIP, device=DEV)
    names = set()
    for s in range(steps):
        _lib.check(lib.nic_ensemble_adam_prepare_clipped(K, P, t["hyper"].data_ptr(), t["max_norm"].data_ptr(), t["state"].data_ptr(),
                                                         t["coef"].data_ptr(), t["grads"][s].data_ptr(), grads.shape[2],
                                                         t["clip"][s].data_ptr(), stream))
        names.add(lib.nic_last_kernel().decode())
        _lib.check(lib.nic_ensemble_adam_update_clipped(K, P, t["params"].data_ptr(), params.shape[1], t["grads"][s].data_ptr(),
                                                        grads.shape[2], t["exp_avg"].data_ptr(), exp_avg.shape[1],
                                                        t["exp_avg_sq"].data_ptr(), exp_avg_sq.shape[1], t["coef"].data_ptr(),
                                                        t["clip"][s].data_ptr(), stream))
        names.add(lib.nic_last_kernel().decode())
    torch.cuda.synchronize()
    assert names == {f"ensemble_adam_prepare_clipped<{P},models={K}>", f"ensemble_adam_update_clipped<{P},models={K}>"}
    assert t["grads"].cpu().numpy().tobytes() == np.ascontiguousarray(grads).tobytes()   # (read only)
    out = {k: t[k].cpu().numpy() for k in ("params", "exp_avg", "exp_avg_sq", "coef", "clip")}
    out["state"] = np.frombuffer(t["state"].cpu().numpy().tobytes(), dtype=eac.STATE_DTYPE)
    return out


KEYS = ("params", "exp_avg", "exp_avg_sq", "coef", "clip", "state")


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("K", [1, 3])
def test_kernels_equal_the_host_build_of_the_body_bit_for_bit(harness, K, P):
    """relies on -ffp-contract=off, IEEE double +, *, / and sqrt, correctly rounded float division and square root, the header's
    order of the additions and inputs that produce no denormals (test_ensemble_clip_host.py checks the last)"""
    exe, d = harness
    args = _padded_inputs(P, list(range(K)))
    got, want = _device_steps(P, *args), ecc.run_harness(exe, d, P, *args)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k   # (live columns and the NaN of every gap, bit for bit)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert np.isfinite(got[k][:, :P]).all() and np.isnan(got[k][:, P:]).all(), k
    assert list(got["state"]["step"]) == [eac.STEPS] * K and np.isfinite(got["clip"]).all()
    assert (ecc.ulps32(got["clip"][:, :, 1], ecc.norms_f64(eac.inputs(P)[1][:, :K])) <= 1.0).all()


@pytest.mark.parametrize("P", [257, 2305])
def test_a_row_of_three_equals_a_launch_of_one_on_that_row(P):
    three = _device_steps(P, *_padded_inputs(P, [0, 1, 2]))
    assert (three["clip"][:, 1, 0] < 1).any() and (three["clip"][:, 2, 0] == 1).all()
    for m in range(3):
        one = _device_steps(P, *_padded_inputs(P, [m]))
        for k in KEYS:
            a = three[k][:, m:m + 1] if k == "clip" else three[k][m:m + 1]
            assert np.ascontiguousarray(a).tobytes() == one[k].tobytes(), (k, m)


@pytest.mark.parametrize("what", ["no_models", "too_many_models", "no_columns", "null_grads", "null_state", "null_max_norm", "null_clip",
                                  "short_params_stride", "short_grads_stride", "short_exp_avg_stride", "short_exp_avg_sq_stride"])
def test_refused_requests_launch_nothing(what):
    """non-zero status, a message, and the poisoned buffers unchanged"""
    K, P, POISON = 3, 257, -12345.0
    buf = {k: torch.full((K, P), POISON, device=DEV) for k in ("params", "grads", "exp_avg", "exp_avg_sq")}
    hyper = torch.tensor(eac.HYPER, dtype=torch.float64, device=DEV)
    max_norm = torch.tensor(ecc.MAX_NORMS, dtype=torch.float64, device=DEV)
    state = torch.full((K, 3), POISON, dtype=torch.float64, device=DEV)
    coef = torch.full((K, eac.N_COEF), POISON, device=DEV)
    clip = torch.full((K, ecc.N_CLIP), POISON, device=DEV)
    n, cols = {"no_models": (0, P), "too_many_models": (65536, P), "no_columns": (K, 0)}.get(what, (K, P))
    stride = {k: P - 1 if what == f"short_{k}_stride" else P for k in buf}
    ptr = {k: None if what == f"null_{k}" else t.data_ptr() for k, t in dict(buf, state=state, max_norm=max_norm, clip=clip).items()}
    lib, stream = _lib.lib(), _lib.current_stream()
    if what not in ("short_params_stride", "short_exp_avg_stride", "short_exp_avg_sq_stride"):
        assert lib.nic_ensemble_adam_prepare_clipped(n, cols, hyper.data_ptr(), ptr["max_norm"], ptr["state"], coef.data_ptr(), ptr["grads"],
                                                     stride["grads"], ptr["clip"], stream) != 0
        assert lib.nic_last_error().decode().startswith("nic_ensemble_adam_prepare_clipped:")
    if what not in ("null_state", "null_max_norm"):
        assert lib.nic_ensemble_adam_update_clipped(n, cols, ptr["params"], stride["params"], ptr["grads"], stride["grads"], ptr["exp_avg"],
                                                    stride["exp_avg"], ptr["exp_avg_sq"], stride["exp_avg_sq"], coef.data_ptr(), ptr["clip"],
                                                    stream) != 0
        assert lib.nic_last_error().decode().startswith("nic_ensemble_adam_update_clipped:")
    torch.cuda.synchronize()
    for k, t in dict(buf, state=state, coef=coef, clip=clip).items():
        assert bool((t == POISON).all()), k


# ---- optimizer level -----------------------------------------------------------------------------------------------------------------
def _optimizer_steps(max_grad_norm, P=2305, steps=3):
    params, grads, hyper = eac.inputs(P)
    opt = EnsembleAdam(3, P, DEV, lr=hyper[:, 0].tolist(), betas=(hyper[:, 1].tolist(), hyper[:, 2].tolist()), eps=hyper[:, 3].tolist(),
                       weight_decay=hyper[:, 4].tolist(), max_grad_norm=max_grad_norm)
    p = torch.from_numpy(eac.padded(params, P + 3)).to(DEV)
    g = torch.from_numpy(eac.padded(grads[:steps], P + 5)).to(DEV)
    seen = []
    for s in range(steps):
        opt.step(p, g[s])
        seen.append(dict(opt.last_kernels))
    torch.cuda.synchronize()
    return opt, p, seen, grads[:steps]


def test_an_optimizer_without_a_max_norm_launches_the_two_old_kernels():
    opt, _, seen, _ = _optimizer_steps(None)
    assert all(k == {"prepare": "ensemble_adam_prepare<models=3>", "update": "ensemble_adam_update<2305,models=3>"} for k in seen)
    assert opt.max_norm is None and opt.clip is None and opt.capture_key()[0] is False and len(opt.capture_key()) == 6


def test_rows_that_are_not_clipped_are_the_unclipped_optimizers_bits():
    plain, p_plain, _, _ = _optimizer_steps(None)
    opt, p, seen, grads = _optimizer_steps([INF, 1.0, 1e6])
    assert all(k == {"prepare": "ensemble_adam_prepare_clipped<2305,models=3>", "update": "ensemble_adam_update_clipped<2305,models=3>"}
               for k in seen)
    for m, same in enumerate((True, False, True)):
        for a, b in ((p, p_plain), (opt.exp_avg, plain.exp_avg), (opt.exp_avg_sq, plain.exp_avg_sq)):
            assert _bits(a[m], b[m]) == same, m
    assert _bits(opt.state, plain.state) and _bits(opt.coef, plain.coef)
    assert bool(torch.isnan(p[:, 2305:]).all())
    norms, scales = opt.grad_norms.cpu().numpy(), opt.clip_scales.cpu().numpy()
    want = ecc.norms_f64(grads[-1])
    assert (ecc.ulps32(norms, want) <= 1.0).all() and (ecc.ulps32(scales, ecc.scales_f64(want, [INF, 1.0, 1e6])) <= 1.0).all()
    assert scales[0] == 1.0 and scales[1] < 1.0 and scales[2] == 1.0
    assert opt.grad_norms.data_ptr() == opt.clip.data_ptr() + 4


# ---- engine level: test_gpu_ensemble_adam's cfg1 workload ------------------------------------------------------------------------------
B, T, IGNORE, LRS = tga.B, tga.T, tga.IGNORE, tga.LRS
# per model: not clipped; far below any gradient norm of this workload (every step is clipped: the tests assert it); never reached
CLIPS = (INF, 1e-3, 1e9)
CLIPS_LATER = (1e-3, INF, 2e-3)   # what `set_max_grad_norm` sets between steps 3 and 4


def _optimizer(ens, clips=CLIPS, lrs=LRS):
    P = sum(p.numel() for p in ens.models[0].parameters())
    return EnsembleAdam(len(tga.SEEDS), P, DEV, lr=lrs, param_shapes=ens.param_shapes or [p.shape for p in ens.models[0].parameters()],
                        max_grad_norm=clips)


def _snapshot(ens, opt, totals, clips):
    return dict(tga._snapshot(ens, opt, totals), clip=torch.stack(clips))


def _train(use_graph=False, clips=CLIPS, change=None, steps=5):
    """`change`: (step, max norms) set before that step"""
    ens = tga._engine(use_graph=use_graph)
    opt = _optimizer(ens, clips)
    obs, totals, seen = tga._workload()[2], [], []
    for i, data in enumerate(tga._batches()[:steps]):
        if change is not None and i == change[0]:
            opt.set_max_grad_norm(change[1])
        totals.append(torch.stack(ens.train_step(data, T, IGNORE, opt, obs)))
        seen.append(opt.clip.clone() if opt.clip is not None else torch.ones(len(tga.SEEDS), 2, device=DEV))
    return ens, opt, _snapshot(ens, opt, totals, seen)


@functools.lru_cache(maxsize=None)
def _eager(clips=CLIPS, change=None):
    """the eager runs the other routes are held to: computed once, read only"""
    return _train(False, clips, change)[2]


def _assert_same(got, want):
    for k in want:
        assert _bits(got[k], want[k]), k


def _assert_clipped_as_planned(clip, clips=CLIPS):
    """[steps][K][2]: a model with an infinite or unreachable max norm has scale 1, the one far below the norms is scaled every step"""
    scales = clip[:, :, 0].cpu()
    assert bool(torch.isfinite(clip).all()) and bool((clip[:, :, 1] > 0).all())
    for m, c in enumerate(clips):
        assert bool((scales[:, m] == 1).all()) if c in (INF, 1e9) else bool((scales[:, m] < 1).all()), (m, scales[:, m])


def test_train_step_equals_run_then_step_on_an_unbound_twin():
    want = _eager()
    _assert_clipped_as_planned(want["clip"])
    twin = tga._engine(bound=False)
    opt, obs, totals, seen = _optimizer(twin), tga._workload()[2], [], []
    for data in tga._batches():
        totals.append(torch.stack(twin.run(data, T, IGNORE, train=True, observation_params=obs)))
        opt.step(twin.weights, twin.grad)
        seen.append(opt.clip.clone())
        tga._write_back(twin)
    _assert_same(_snapshot(twin, opt, totals, seen), want)
    assert opt.steps().tolist() == [5, 5, 5]
    assert (opt.last_kernels["prepare"], opt.last_kernels["update"]) == ("ensemble_adam_prepare_clipped<2305,models=3>",
                                                                         "ensemble_adam_update_clipped<2305,models=3>")
    # clipping did something to model 1 and nothing to the others
    plain = tga._eager()
    for m, same in enumerate((True, False, True)):
        assert _bits(want["weights"][m], plain["weights"][m]) == same, m


def _clipped(grads, clips):
    """[K][P] device float32 -> the clipped gradients in float64 (a tensor `_referee` passes through to the float64 Adam)"""
    return torch.from_numpy(ecc.clipped_f64(grads.cpu().numpy()[None], clips)[0])


def test_first_step_against_three_clip_grad_norms_and_torch_adams():
    theirs = tga._engine(bound=False)
    opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(theirs.models, LRS)]
    ours = tga._engine()
    opt, obs, data = _optimizer(ours), tga._workload()[2], tga._batches()[0]
    params0 = ours.weights.clone()
    assert torch.equal(params0, tga._packed(theirs.models))
    P = params0.shape[1]
    ours.train_step(data, T, IGNORE, opt, obs)
    theirs.run(data, T, IGNORE, train=True, observation_params=obs)
    assert _bits(ours.grad, theirs.grad)
    returned = [float(torch.nn.utils.clip_grad_norm_(m.parameters(), c)) for m, c in zip(theirs.models, CLIPS)]
    for o in opts:
        o.step()
    grads = ours.grad[:, :P]
    tga._referee(params0, _clipped(grads, CLIPS), np.array([[lr, 0.9, 0.999, 1e-8, 0.0] for lr in LRS]), ours.weights,
                 tga._packed(theirs.models), "clipped step 1")
    want = ecc.norms_f64(grads.cpu().numpy())
    norms, scales = opt.grad_norms.cpu().numpy(), opt.clip_scales.cpu().numpy()
    print("norms", norms, "float64", want, "clip_grad_norm_", returned, "scales", scales)
    assert (ecc.ulps32(norms, want) <= 1.0).all() and (ecc.ulps32(scales, ecc.scales_f64(want, CLIPS)) <= 1.0).all()
    assert np.allclose(norms, returned, rtol=1e-5, atol=0)
    assert scales[0] == 1.0 and scales[1] < 1.0 and scales[2] == 1.0


# ---- replay ----------------------------------------------------------------------------------------------------------------------------
def test_replayed_steps_equal_eager_steps():
    ens, opt, got = _train(use_graph=True)
    _assert_same(got, _eager())
    assert len(ens._graphs) > 0 and opt.steps().tolist() == [5, 5, 5]


def test_a_new_max_norm_reaches_a_replayed_step():
    change = (3, CLIPS_LATER)
    ens, opt, got = _train(use_graph=True, change=change)
    assert len(ens._graphs) == 1   # (one capture served the steps before and after the change)
    _assert_same(got, _eager(change=change))
    _assert_clipped_as_planned(got["clip"][:3])
    _assert_clipped_as_planned(got["clip"][3:], CLIPS_LATER)
    assert not _bits(got["weights"], _eager()["weights"])   # (the change did something)


def test_clipping_enabled_after_an_unclipped_capture_is_not_served_by_it():
    change = (3, CLIPS)
    ens, opt, got = _train(use_graph=True, clips=None, change=change)
    assert len(ens._graphs) == 2   # (the unclipped capture, then one of the clipped launches)
    _assert_same(got, _eager(clips=None, change=change))
    _assert_clipped_as_planned(got["clip"][3:])
    assert opt.last_kernels["update"] == "ensemble_adam_update_clipped<2305,models=3>"
    assert not _bits(got["weights"][1], tga._eager()["weights"][1]) and _bits(got["weights"][0], tga._eager()["weights"][0])


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------------
def test_a_checkpointed_clipped_run_equals_an_uninterrupted_one():
    """the clip value is not Adam state: the fresh optimizer is given it again, everything else comes from the checkpoint"""
    ens = tga._engine()
    opt, obs, batches, totals, seen = _optimizer(ens), tga._workload()[2], tga._batches(), [], []
    for data in batches[:3]:
        totals.append(torch.stack(ens.train_step(data, T, IGNORE, opt, obs)))
        seen.append(opt.clip.clone())
    sds = [opt.state_dict(m) for m in range(3)]
    assert all("max_grad_norm" not in sd["param_groups"][0] for sd in sds)
    fresh = _optimizer(ens, lrs=1.0)
    for m, sd in enumerate(sds):
        fresh.load_state_dict(m, copy.deepcopy(sd))
    assert fresh.max_norm.tolist() == list(CLIPS)
    for data in batches[3:]:
        totals.append(torch.stack(ens.train_step(data, T, IGNORE, fresh, obs)))
        seen.append(fresh.clip.clone())
    _assert_same(_snapshot(ens, fresh, totals, seen), _eager())


# ---- make_optimizer --------------------------------------------------------------------------------------------------------------------
def test_make_optimizer_picks_up_the_models_clipping_values():
    ens = tga._engine(bound=False)
    with pytest.raises(ValueError, match="needs sized weights"):
        ens.make_optimizer(LRS)
    ens.bind_parameters()
    for m, c in zip(ens.models, CLIPS):
        m.gradient_clipping_norm_value = None if c == INF else c
    opt = ens.make_optimizer(LRS)
    assert isinstance(opt, EnsembleAdam) and (opt.n_models, opt.P) == tuple(ens.weights.shape) and opt.max_norm.tolist() == list(CLIPS)
    assert [tuple(s) for s in opt.param_shapes] == [tuple(p.shape) for p in ens.models[0].parameters()]
    obs, totals, seen = tga._workload()[2], [], []
    for data in tga._batches():
        totals.append(torch.stack(ens.train_step(data, T, IGNORE, opt, obs)))
        seen.append(opt.clip.clone())
    _assert_same(_snapshot(ens, opt, totals, seen), _eager())
    for m in ens.models:
        m.gradient_clipping_norm_value = None
    assert ens.make_optimizer(LRS).max_norm is None and ens.make_optimizer(LRS, max_grad_norm=2.0).max_norm.tolist() == [2.0] * 3


# ---- the same on K data_driven policies ------------------------------------------------------------------------------------------------
def _horizon():
    s = ths._setting(ths.base.ENGINE_CASES[0])
    return s, lambda ens: EnsembleAdam(ens.n_models, ens.weights.shape[1], DEV, lr=list(ths.LRS), param_shapes=ens.param_shapes,
                                       max_grad_norm=CLIPS)


def test_horizon_train_step_equals_run_then_step_on_a_twin():
    s, optimizer = _horizon()
    ours, twin = s.engine(), s.engine()
    opt, opt_twin = optimizer(ours), optimizer(twin)
    plain = s.engine()
    opt_plain = s.optimizer(plain)
    for _ in range(3):
        got = s.step(ours, opt)
        want = s.run(twin)
        opt_twin.step(twin.weights, twin.grad)
        s.step(plain, opt_plain)
        assert _bits(got[0], want[0]) and _bits(got[1], want[1])
        assert _bits(opt.clip, opt_twin.clip)
        _assert_clipped_as_planned(opt.clip[None])
    torch.cuda.synchronize()
    assert _bits(ours.weights, twin.weights) and _bits(ours.grad, twin.grad)
    assert _bits(opt.exp_avg, opt_twin.exp_avg) and _bits(opt.exp_avg_sq, opt_twin.exp_avg_sq) and _bits(opt.state, opt_twin.state)
    assert opt.steps().tolist() == [3, 3, 3] and bool(torch.isfinite(ours.weights).all())
    P = ours.weights.shape[1]
    assert opt.last_kernels == {"prepare": f"ensemble_adam_prepare_clipped<{P},models=3>", "update": f"ensemble_adam_update_clipped<{P},models=3>"}
    for m, same in enumerate((True, False, True)):
        assert _bits(ours.weights[m], plain.weights[m]) == same, m


def test_horizon_first_step_against_clip_grad_norm_and_torch_adam():
    s, optimizer = _horizon()
    ours, theirs = s.engine(), s.engine(bound=False)
    opt = optimizer(ours)
    opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(theirs.models, ths.LRS)]
    params0 = ours.weights.clone()
    assert _bits(params0, ths._packed(theirs.models))
    s.step(ours, opt)
    s.run(theirs)
    assert _bits(ours.grad, theirs.grad)
    returned = [float(torch.nn.utils.clip_grad_norm_(m.parameters(), c)) for m, c in zip(theirs.models, CLIPS)]
    for o in opts:
        o.step()
    P = params0.shape[1]
    grads = ours.grad[:, :P]
    tga._referee(params0, _clipped(grads, CLIPS), np.array([[lr, 0.9, 0.999, 1e-8, 0.0] for lr in ths.LRS]), ours.weights,
                 ths._packed(theirs.models), "horizon, clipped step 1")
    want = ecc.norms_f64(grads.cpu().numpy())
    norms, scales = opt.grad_norms.cpu().numpy(), opt.clip_scales.cpu().numpy()
    print("norms", norms, "float64", want, "clip_grad_norm_", returned, "scales", scales)
    assert (ecc.ulps32(norms, want) <= 1.0).all() and (ecc.ulps32(scales, ecc.scales_f64(want, CLIPS)) <= 1.0).all()
    assert np.allclose(norms, returned, rtol=1e-5, atol=0)
    assert scales[0] == 1.0 and scales[1] < 1.0 and scales[2] == 1.0
