"""Stopped models leave the data_driven K-model launches, on a real MI355X: the active-model mask of
`nic_horizon_rollout_ensemble_* / _instances_*_active`, `nic_linear_fwd_models_active`, `nic_linear_wgrad_models_active`,
`nic_wgrad_reduce_models_active`, `HorizonPolicyEnsemble.skip_inactive` and `fit(trainer_params=...)` on that engine.

The contract is one sentence, and the bar is bits: a model whose entry is zero has NO byte of its slices read or written - every
output is prefilled with a sentinel (a NaN pattern: a value that was read would also poison what is compared) and must still hold
it -, and a model that runs gets the bits of the entry point without a mask.  K = 3 throughout."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_gpu_horizon as single  # noqa: E402
import test_gpu_horizon_ensemble as ens  # noqa: E402  (_Launch: K models' weights and buffers with NaN gaps; KERNEL_CASES)
import test_gpu_horizon_ensemble_step as hz_step  # noqa: E402  (_setting: a fixture's batch, engine and optimizer)
import test_gpu_horizon_instances as inst  # noqa: E402  (_Launch on I instances; _instance_batch)
import test_gpu_linear_models as lm  # noqa: E402  (the shapes that reach every kernel with a model form)
from neural_inventory_control_amd import _lib, ops  # noqa: E402
from neural_inventory_control_amd import horizon_rollout as hz  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = single.DEV
K = 3
MASKS = ([1, 0, 1], [0, 0, 1], [1, 1, 1])
HISTORIES, DZ = ens.HISTORIES, ens.DZ
NAN = float("nan")


def _bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)   # (also 0-dim: one model's total)
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _mask(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _kernel():
    return _lib.lib().nic_last_kernel().decode()


# ---- 1. the launch pair ------------------------------------------------------------------------------------------------------------
PAIRS = ("ensemble", "instances-I1", "instances-I3")


def _launch(c, pair):
    if pair == "ensemble":
        return ens._Launch(c, K)
    return inst._Launch(c, K, 1 if pair == "instances-I1" else 3)   # (I = 3: one replica per instance)


def _run_pair(E, pair, active):
    """forward + backward through the wrappers (None: the entry points without a mask); the two recorded names"""
    h, dz = [E.hist[n].buf for n in HISTORIES], [E.dz[n].buf for n in DZ]
    if pair == "ensemble":
        hz.horizon_ensemble_fwd(E.desc, E.ens, E.z1_obs.buf, E.L.state0, E.rewards.buf, E.state_final.buf, *h, active=active)
        fwd = _kernel()
        hz.horizon_ensemble_bwd(E.desc, E.ens, *h, E.L.g_reward, *dz, active=active)
    else:
        hz.horizon_instances_fwd(E.desc, E.ens, E.inst, E.z1_obs.buf, E.state0, E.rewards.buf, E.state_final.buf, *h, active=active)
        fwd = _kernel()
        hz.horizon_instances_bwd(E.desc, E.ens, E.inst, *h, E.L.g_reward, *dz, active=active)
    bwd = _kernel()
    torch.cuda.synchronize()
    return fwd, bwd


_UNMASKED = {}


def _unmasked(c, pair):
    """({output: the whole buffer after the unmasked pair}, its names): computed once per (case, pair), shared, never modified"""
    if (c.id, pair) not in _UNMASKED:
        E = _launch(c, pair)
        names = _run_pair(E, pair, None)
        _UNMASKED[c.id, pair] = ({n: b.buf.clone() for n, b in E.outputs.items()}, names)
    return _UNMASKED[c.id, pair]


@pytest.mark.parametrize("mask", MASKS, ids=lambda m: "".join(map(str, m)))
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("c", ens.KERNEL_CASES, ids=[c.id for c in ens.KERNEL_CASES])
def test_masked_pair_leaves_stopped_models_alone_and_gives_the_others_the_unmasked_bits(c, pair, mask):
    want, (want_fwd, want_bwd) = _unmasked(c, pair)
    assert "active" not in want_fwd + want_bwd and f"models={K}" in want_fwd and f"models={K}" in want_bwd
    E = _launch(c, pair)
    sentinel = {n: b.buf.clone() for n, b in E.outputs.items()}   # (every output is NaN-filled by _Launch)
    assert all(bool(torch.isnan(t).all()) for t in sentinel.values())
    fwd, bwd = _run_pair(E, pair, _mask(mask))
    assert fwd == want_fwd[:-1] + ",active>" and bwd == want_bwd[:-1] + ",active>", (fwd, bwd)
    for n, b in E.outputs.items():
        for m in range(K):
            lo, hi = m * b.stride, (m + 1) * b.stride
            if mask[m]:
                assert _bits(b.buf[lo:hi], want[n][lo:hi]), (c.id, pair, n, m, "an active model's bits moved")
                assert not bool(torch.isnan(b.live(m)).any()), (c.id, pair, n, m)
            else:
                assert _bits(b.buf[lo:hi], sentinel[n][lo:hi]), (c.id, pair, n, m, "a stopped model's slice was written")
    assert E.inputs_unchanged()


def test_null_mask_runs_every_model():
    """NULL through the `_active` entry points: accepted, every model runs (the rule of the small kernels' entry points)"""
    lib, p = _lib.lib(), _lib.ptr
    c = single._case("ref")
    want, _ = _unmasked(c, "ensemble")
    E = ens._Launch(c, K)
    h, dz = [p(E.hist[n].buf) for n in HISTORIES], [p(E.dz[n].buf) for n in DZ]
    assert lib.nic_horizon_rollout_ensemble_fwd_active(E.desc, E.ens, p(E.z1_obs.buf), p(E.L.state0), p(E.rewards.buf), p(E.state_final.buf),
                                                       *h, None, _lib.current_stream()) == 0, lib.nic_last_error()
    assert _kernel().endswith(",active>")
    assert lib.nic_horizon_rollout_ensemble_bwd_active(E.desc, E.ens, *h, E.L.g_reward.t2(), *dz, None, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert all(_bits(b.buf, want[n]) for n, b in E.outputs.items())


# ---- 2. the GEMMs --------------------------------------------------------------------------------------------------------------------
def _up4(n):
    return (n + 3) // 4 * 4


def _check_masked(out, want, start, stride, mask, what):
    for m in range(K):
        lo, hi = m * stride, (m + 1) * stride
        if mask[m]:
            assert _bits(out[lo:hi], want[lo:hi]), (what, m, "an active model's bits moved")
        else:
            assert _bits(out[lo:hi], start[lo:hi]), (what, m, "a stopped model's slice was written")


def _fwd_masked(case, masks=MASKS):
    """test_gpu_linear_models._fwd_case's layout (strides = slice + gap, NaN in every gap and padding column) under each mask,
    against the entry point without a mask on the same operands; returns the single-model kernel's name"""
    N, Kc, cols, ldw, act, with_bias, shared = case
    lib, stream = lm._lib_stream()
    ldb = cols + 8
    sW, sB, sX, sY = _up4(N * ldw) + lm.GAP, N + 3, Kc * ldb + lm.GAP, N * ldb + lm.GAP
    W, X = 0.1 * lm._rand(K * sW, 1), lm._rand(K * sX, 2)
    bias = lm._rand(K * sB, 3) if with_bias else None
    start = torch.full((K * sY,), NAN, device="cuda")
    want = start.clone()
    _lib.check(lib.nic_linear_fwd_models(lm._p(W), ldw, sW, lm._p(bias), sB, lm._p(X), 0 if shared else sX, lm._p(want), sY, N, Kc, cols,
                                         ldb, act, K, stream))
    unmasked = _kernel()
    assert unmasked.endswith(f",models={K}>")
    for mask in masks:
        Y = start.clone()
        _lib.check(lib.nic_linear_fwd_models_active(lm._p(W), ldw, sW, lm._p(bias), sB, lm._p(X), 0 if shared else sX, lm._p(Y), sY, N, Kc,
                                                    cols, ldb, act, K, lm._p(_mask(mask)), stream))
        assert _kernel() == unmasked[:-1] + ",active>", _kernel()
        torch.cuda.synchronize()
        _check_masked(Y, want, start, sY, mask, ("fwd", case, mask))
    return lm._single_name(unmasked)


def _wgrad_masked(shape, cols=140, n_splits=3, masks=MASKS):
    N, Kc, off = shape
    lib, stream = lm._lib_stream()
    ldb, lds = cols, _up4(Kc + 1)
    s_dy, s_x, s_slab = N * ldb + lm.GAP, Kc * ldb + lm.GAP, n_splits * N * lds + lm.GAP
    dY, Xbuf = lm._rand(K * s_dy, 4), lm._rand(K * s_x + 4, 5)
    start = torch.full((K, s_slab), NAN, device="cuda")   # (the contraction ADDS: values in the live elements, NaN around them)
    start[:, :n_splits * N * lds].view(K, n_splits * N, lds)[:, :, :Kc + 1] = lm._rand(K * n_splits * N * (Kc + 1), 6).view(K, n_splits * N, Kc + 1)
    start = start.view(-1)
    want = start.clone()
    _lib.check(lib.nic_linear_wgrad_models(lm._p(dY), s_dy, lm._p(Xbuf, off), s_x, lm._p(want), s_slab, lds, N, Kc, cols, ldb, n_splits, K, stream))
    unmasked = _kernel()
    assert unmasked.endswith(f",models={K}>")
    for mask in masks:
        slab = start.clone()
        _lib.check(lib.nic_linear_wgrad_models_active(lm._p(dY), s_dy, lm._p(Xbuf, off), s_x, lm._p(slab), s_slab, lds, N, Kc, cols, ldb,
                                                      n_splits, K, lm._p(_mask(mask)), stream))
        assert _kernel() == unmasked[:-1] + ",active>", _kernel()
        torch.cuda.synchronize()
        _check_masked(slab, want, start, s_slab, mask, ("wgrad", shape, mask))
    assert not _bits(want, start)
    return lm._single_name(unmasked)


def _reduce_masked(n_splits, masks=MASKS):
    N, Kc = 17, 33
    lib, stream = lm._lib_stream()
    lds, lddw = _up4(Kc + 1), Kc + 3
    s_slab, s_dw, s_db = n_splits * N * lds + lm.GAP, N * lddw + 5, N + 3
    slab = lm._rand(K * s_slab, 7)
    start_w, start_b = torch.full((K * s_dw,), NAN, device="cuda"), torch.full((K * s_db,), NAN, device="cuda")
    want_w, want_b = start_w.clone(), start_b.clone()
    _lib.check(lib.nic_wgrad_reduce_models(lm._p(slab), s_slab, lds, n_splits, lm._p(want_w), lddw, s_dw, lm._p(want_b), s_db, N, Kc, 0.5, K, stream))
    unmasked = _kernel()
    assert unmasked.endswith(f",models={K}")
    for mask in masks:
        dW, db = start_w.clone(), start_b.clone()
        _lib.check(lib.nic_wgrad_reduce_models_active(lm._p(slab), s_slab, lds, n_splits, lm._p(dW), lddw, s_dw, lm._p(db), s_db, N, Kc, 0.5, K,
                                                      lm._p(_mask(mask)), stream))
        assert _kernel() == unmasked + ",active", _kernel()
        torch.cuda.synchronize()
        _check_masked(dW, want_w, start_w, s_dw, mask, ("reduce dW", n_splits, mask))
        _check_masked(db, want_b, start_b, s_db, mask, ("reduce db", n_splits, mask))
    return lm._single_name(unmasked)


@pytest.mark.parametrize("case", lm.FWD_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_masked_forward_gemm(case):
    _fwd_masked(case)


@pytest.mark.parametrize("shape", lm.WGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_masked_weight_gradient_gemm(shape):
    _wgrad_masked(shape)


@pytest.mark.parametrize("n_splits", [3, 130])
def test_masked_reduce(n_splits):
    _reduce_masked(n_splits)


def test_every_model_form_has_run_masked_and_no_other():
    one = (MASKS[0],)
    reached = ({_fwd_masked(case, one) for case in lm.FWD_CASES} | {_wgrad_masked(shape, masks=one) for shape in lm.WGRAD_SHAPES}
               | {_reduce_masked(n, one) for n in (3, 130)})
    assert reached == lm.FWD_KERNELS | lm.WGRAD_KERNELS | {"wgrad_reduce_kernel", "wgrad_reduce_wide_kernel"}


def test_ops_wrappers_pass_the_mask_and_refuse_a_tensor_that_is_not_one():
    M, N, Kc, cols = K, 17, 41, 140
    W, bias, X = 0.1 * lm._rand(M * N * 44, 8).view(M, N, 44), lm._rand(M * N, 9).view(M, N), lm._rand(M * Kc * cols, 10).view(M, Kc, cols)
    Y, want = torch.full((M, N, cols), NAN, device="cuda"), torch.full((M, N, cols), NAN, device="cuda")
    ops.linear_fwd_models(W[:, :, :Kc], bias, X[0], want, cols, _lib.NIC_ACT_ELU)
    ops.linear_fwd_models(W[:, :, :Kc], bias, X[0], Y, cols, _lib.NIC_ACT_ELU, active=_mask([1, 0, 1]))
    assert _kernel().endswith(",active>")
    assert _bits(Y[0], want[0]) and _bits(Y[2], want[2]) and bool(torch.isnan(Y[1]).all())
    for bad in (torch.ones(2, dtype=torch.int32, device="cuda"), torch.ones(3, dtype=torch.int64, device="cuda"),
                torch.ones(3, dtype=torch.int32), torch.ones(6, dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(ValueError, match="the active mask must be a contiguous int32"):
            ops.linear_fwd_models(W[:, :, :Kc], bias, X[0], Y, cols, _lib.NIC_ACT_ELU, active=bad)
    assert _bits(Y[0], want[0]) and bool(torch.isnan(Y[1]).all())


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_a_misaligned_mask_is_refused_by_all_seven_and_nothing_is_launched():
    lib, p, stream = _lib.lib(), _lib.ptr, _lib.current_stream()
    reason = "the active mask must be NULL or 4-byte aligned"
    bad = torch.ones(K + 1, dtype=torch.int32, device=DEV).data_ptr() + 2   # (an address inside a live allocation, 2 bytes off)
    c = single._case("ref")
    E = inst._Launch(c, K, 3)
    h, dz = [p(E.hist[n].buf) for n in HISTORIES], [p(E.dz[n].buf) for n in DZ]
    fwd_args = (p(E.z1_obs.buf), p(E.state0), p(E.rewards.buf), p(E.state_final.buf), *h)
    bwd_args = (*h, E.L.g_reward.t2(), *dz)
    calls = [("nic_horizon_rollout_ensemble_fwd_active", (E.desc, E.ens) + fwd_args),
             ("nic_horizon_rollout_ensemble_bwd_active", (E.desc, E.ens) + bwd_args),
             ("nic_horizon_rollout_instances_fwd_active", (E.desc, E.ens, E.inst) + fwd_args),
             ("nic_horizon_rollout_instances_bwd_active", (E.desc, E.ens, E.inst) + bwd_args)]
    for name, args in calls:
        assert getattr(lib, name)(*args, bad, stream) != 0, name
        message = lib.nic_last_error().decode()
        assert message.startswith(name + ":") and reason in message, message
    torch.cuda.synchronize()
    assert all(b.all_untouched() for b in E.outputs.values())
    # the three GEMM entry points (the layout of test_gpu_linear_models' refusal test)
    M, N, Kc, cols = K, 17, 41, 140
    ldw, ldb, lds, lddw, n_splits = 44, cols, 44, Kc, 3
    sW, sB, sX, sY = N * ldw + lm.GAP, N + 3, Kc * ldb + lm.GAP, N * ldb + lm.GAP
    s_slab, s_dw, s_db = n_splits * N * lds + lm.GAP, N * lddw + 5, N + 3
    W, bias, X, dY = 0.1 * lm._rand(M * sW, 12), lm._rand(M * sB, 13), lm._rand(M * sX + 4, 14), lm._rand(M * sY, 15)
    nan = lambda n: torch.full((n,), NAN, device="cuda")   # noqa: E731
    Y, slab, dW, db = nan(M * sY), nan(M * s_slab), nan(M * s_dw), nan(M * s_db)
    q = lm._p
    gemms = [("nic_linear_fwd_models_active", (q(W), ldw, sW, q(bias), sB, q(X), sX, q(Y), sY, N, Kc, cols, ldb, _lib.NIC_ACT_ELU, M)),
             ("nic_linear_wgrad_models_active", (q(dY), sY, q(X), sX, q(slab), s_slab, lds, N, Kc, cols, ldb, n_splits, M)),
             ("nic_wgrad_reduce_models_active", (q(slab), s_slab, lds, n_splits, q(dW), lddw, s_dw, q(db), s_db, N, Kc, 1.0, M))]
    for name, args in gemms:
        assert getattr(lib, name)(*args, bad, stream) != 0, name
        assert lib.nic_last_error().decode() == "%s: %s" % (name, reason)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (Y, slab, dW, db))
    # the same buffers, the same calls with a good mask
    good = p(_mask([1, 0, 1]))
    slab.zero_()
    for name, args in gemms:
        assert getattr(lib, name)(*args, good, stream) == 0, (name, lib.nic_last_error())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Y.view(M, sY)[0, :N * ldb]).any()) and bool(torch.isnan(Y.view(M, sY)[1]).all())
    assert not bool(torch.isnan(dW.view(M, s_dw)[2, :N * lddw]).any()) and bool(torch.isnan(dW.view(M, s_dw)[1]).all())


# ---- 4. the engine -------------------------------------------------------------------------------------------------------------------
STEP_MASKS = ([1, 1, 1], [1, 0, 1], [0, 0, 1])
BATCHED_TAGS = ("fwd", "bwd", "z1", "wgrad0", "reduce0")


def _instance_batch(data, i):
    """instance i of a fixture batch (0: the batch itself), perturbed as test_gpu_horizon_instances._instance_batch perturbs the
    many-warehouse fixture - which is borrowed where the batch has warehouses; a one-store batch has no warehouse entries, and the
    same rule is applied to what it has (the tables keep their layout)"""
    if i == 0 or "initial_warehouse_inventories" in data:
        return inst._instance_batch(data, i)
    gen = torch.Generator().manual_seed(100 + i)
    rand = lambda t: (0.5 + torch.rand(t.shape, generator=gen)).to(t.device)  # noqa: E731
    out = dict(data)
    for k in ("demands", "initial_inventories"):
        out[k] = (data[k] * rand(data[k])).contiguous()
    for k in ("underage_costs", "holding_costs"):
        if data.get(k) is not None:
            out[k] = (data[k] * (inst.COST_SCALE[i] if k == "underage_costs" else 1.0 + 0.5 * i)).contiguous()
    v = data["lead_times"].float()
    out["lead_times"] = torch.where(v > 0, (v - i).clamp_min(1.0), v).to(data["lead_times"].dtype).contiguous()
    return out


def _engine_batch(s, listed):
    if not listed:
        return s.data
    return [_instance_batch(s.data, i) for i in range(K)]   # one instance per model


def _model_rows(e):
    """the buffers a step writes per model, by name: [K][...] tensors (X: its state rows, the kernel's share of it)"""
    out = dict(weights=e.weights, grad=e.grad, rewards=e.rewards, final=e.final, z1=e.z1, X_state=e.X[:, :e.F_dyn])
    out.update({"hist%d" % i: t for i, t in enumerate(e.hist)})
    out.update({"dz%d" % i: t for i, t in enumerate(e.dz)})
    return out


@pytest.mark.parametrize("name,listed,model_gemms", [
    (ens.ENGINE_CASES[0], False, True), (ens.ENGINE_CASES[0], True, True), (ens.ENGINE_CASES[1], False, True),
    (ens.ENGINE_CASES[1], True, True), (ens.ENGINE_CASES[0], False, False)],
    ids=["many-warehouses-dict", "many-warehouses-list", "one-store-dict", "one-store-list", "many-warehouses-dict-loop"])
def test_engine_steps_skip_stopped_models(name, listed, model_gemms):
    s = hz_step._setting(name)
    batch = _engine_batch(s, listed)
    ours, twin = s.engine(model_gemms=model_gemms), s.engine(model_gemms=model_gemms)   # (the twin: the same models from the same seeds)
    ours.skip_inactive = True
    assert twin.skip_inactive is False and _bits(ours.weights, twin.weights)
    opt, topt = s.optimizer(ours), s.optimizer(twin)
    tags = BATCHED_TAGS if model_gemms else ("fwd", "bwd")
    for step, mask in enumerate(STEP_MASKS):
        ours.set_active(mask)
        twin.set_active(mask)
        before = {k: v.clone() for k, v in _model_rows(ours).items()} if step else None   # (sized by the first step)
        got = s.step(ours, opt, batch)
        want = s.step(twin, topt, batch)
        torch.cuda.synchronize()
        assert ours._models_ok, "the fixture's shapes have model forms: the batched route is what this test is about"
        assert all(ours.last_kernels[t].endswith((",active>", ",active")) for t in tags), ours.last_kernels
        assert "models=" in ours.last_kernels["z1"] if model_gemms else "models=" not in ours.last_kernels["z1"]
        assert not any("active" in n for n in twin.last_kernels.values())
        assert opt.last_kernels["update"].endswith(",active>") and topt.last_kernels["update"].endswith(",active>")
        rows, twin_rows = _model_rows(ours), _model_rows(twin)
        for m in range(K):
            if mask[m]:
                for k in ("weights", "grad", "rewards", "final"):
                    assert _bits(rows[k][m], twin_rows[k][m]), (step, m, k)
                assert _bits(got[0][m], want[0][m]) and _bits(got[1][m], want[1][m]) and bool(torch.isfinite(got[0][m]))
            else:
                for k, v in rows.items():
                    assert _bits(v[m], before[k][m]), (step, m, k, "a stopped model's row was written")
                assert bool(torch.isnan(got[0][m])) and bool(torch.isnan(got[1][m]))
        assert bool(torch.isfinite(want[0]).all())   # (the twin still computes every model's costs)
    assert opt.steps().tolist() == topt.steps().tolist() == [2, 1, 3]
    # an evaluation under the mask; then every model again, through the launches without a mask
    total, _ = s.run(ours, batch, train=False)
    assert torch.isnan(total).tolist() == [True, True, False] and ours.last_kernels["fwd"].endswith(",active>")
    ours.set_active(None)
    total, _ = s.step(ours, opt, batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(total).all()) and not any("active" in n for n in ours.last_kernels.values())
    assert not opt.last_kernels["update"].endswith(",active>")


# ---- 5. the default --------------------------------------------------------------------------------------------------------------------
def test_without_skip_inactive_only_the_optimizer_reads_the_mask():
    s = hz_step._setting(ens.ENGINE_CASES[0])
    e = s.engine()
    opt = s.optimizer(e)
    assert e.skip_inactive is False
    e.set_active([1, 0, 1])
    total, reported = s.step(e, opt)
    torch.cuda.synchronize()
    assert not any("active" in n for n in e.last_kernels.values()), e.last_kernels
    assert opt.last_kernels["prepare"].endswith(",active>") and opt.last_kernels["update"].endswith(",active>")
    assert bool(torch.isfinite(total).all()) and bool(torch.isfinite(reported).all())
    # skip_inactive without a mask: the unmasked launches too
    e.set_active(None)
    e.skip_inactive = True
    total, _ = s.step(e, opt)
    assert not any("active" in n for n in e.last_kernels.values()) and bool(torch.isfinite(total).all())


# ---- 6. fit --------------------------------------------------------------------------------------------------------------------------
FIT_LRS = (1e-3, 1e3, 3e-2)   # a small step, an absurd one (its loss never improves on the first epoch's), one in between
TRAINER = {"do_dev_every_n_epochs": 1, "choose_best_model_on": "dev_loss", "early_stopping_patience_epochs": 2,
           "save_model": False, "print_results_every_n_epochs": 1}
EPOCHS = 8
FIT_CASE = ens.ENGINE_CASES[1]   # the smallest of the three settings: one store, 40 scenarios x 12 periods


def _fit_engine(s, which):
    """an engine on the fixture's K models (`which` = slice(None)) or on one of them alone, from the same seeds, with its learning rate"""
    models = ens._models(s.g, s.g.fresh_config())[which]
    e = hz_step.HorizonPolicyEnsemble(models, s.c["problem_params"], DEV)
    e.bind_parameters()
    return e, s.optimizer(e, FIT_LRS[which])


def test_fit_with_early_stopping_equals_one_model_engines_running_the_same_fit():
    s = hz_step._setting(FIT_CASE)
    B = s.data["demands"].shape[0]
    train = [{k: v[:B // 2].contiguous() for k, v in s.data.items()}, {k: v[B // 2:].contiguous() for k, v in s.data.items()}]
    dev = [s.data]
    e, opt = _fit_engine(s, slice(None))
    forward_names = []
    step = e._step

    def noting_step(*args, **kw):   # (the forward's recorded name of every step of the fit, and what skip_inactive was)
        out = step(*args, **kw)
        forward_names.append((e.last_kernels["fwd"], e.skip_inactive, e.active_models().tolist()))
        return out
    e._step = noting_step
    assert e.skip_inactive is False
    train_hist, dev_hist = e.fit(train, dev, EPOCHS, s.T, s.T, s.ignore, opt, s.obs, trainer_params=TRAINER)
    torch.cuda.synchronize()
    assert e.skip_inactive is False   # back at its previous value
    stopped = e.stopped_epoch.tolist()
    early = [v for v in stopped if 0 <= v < EPOCHS - 1]
    assert early, ("no model stopped before the last epoch: the test would pass vacuously", stopped)
    # during the fit every launch took the mask; after the first stop a model really was skipped
    assert all(name.endswith(",active>") and skipping for name, skipping, _ in forward_names), forward_names[:3]
    assert any(not all(active) for _, _, active in forward_names)
    for m in range(K):
        alone, aopt = _fit_engine(s, slice(m, m + 1))
        th, dh = alone.fit(train, dev, EPOCHS, s.T, s.T, s.ignore, aopt, s.obs, trainer_params=TRAINER)
        torch.cuda.synchronize()
        assert int(e.stopped_epoch[m]) == int(alone.stopped_epoch[0]), m
        assert int(e.best_epoch[m]) == int(alone.best_epoch[0]), m
        assert _bits(e.best_dev[m], alone.best_dev[0]) and _bits(e.best_train[m], alone.best_train[0]), m
        assert _bits(e.best_weights[m], alone.best_weights[0]), m
        assert _bits(e.weights[m], alone.weights[0]), m           # the final weights: frozen from the stop on
        assert _bits(train_hist[:, m], th[:, 0]) and _bits(dev_hist[:, m], dh[:, 0]), m
        last = stopped[m] if stopped[m] >= 0 else EPOCHS - 1
        assert bool(torch.isnan(train_hist[last + 1:, m]).all()) and bool(torch.isnan(dev_hist[last + 1:, m]).all())
        assert int(opt.steps()[m]) == 2 * (last + 1)                  # two batches an epoch, none after the stop
    assert e.active_models().tolist() == [v < 0 for v in stopped]
    # fit without trainer_params stays the loop it was: no mask, no skipping
    plain, popt = _fit_engine(s, slice(None))
    plain.fit(train, dev, 1, s.T, s.T, s.ignore, popt, s.obs)
    assert plain.skip_inactive is False and not any("active" in n for n in plain.last_kernels.values())
