"""K data_driven policies in one whole-horizon launch pair (`nic_horizon_rollout_ensemble_fwd / _bwd`, `HorizonPolicyEnsemble`) against K
single-model launches / `FusedRollout.run` steps of the unchanged route, bit for bit.

The single-model kernels are refereed against a float64 rollout by tests/test_gpu_horizon.py (knife edges included); model m of an
ensemble launch runs their instruction stream on its own slice, so the bar here is `torch.equal` - no tolerance - on every output,
plus sentinels in every stride gap, spare row and padding column.  Only the K totals are summed in another (fixed) order than the
single-model route's `torch.sum`: they are held to the project's 1e-5 relative bar."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import horizon_cases as hc  # noqa: E402
import test_gpu_horizon as single  # noqa: E402  (prepare / forward / backward of the single-model kernels: the yardstick)
import test_gpu_rollout as tgr  # noqa: E402  (_model / _load: a fixture's policy on the device)
from golden_io import Golden  # noqa: E402
from neural_inventory_control_amd import _lib  # noqa: E402
from neural_inventory_control_amd import horizon_rollout as hz  # noqa: E402
from neural_inventory_control_amd.horizon_ensemble import HorizonPolicyEnsemble  # noqa: E402
from neural_inventory_control_amd.rollout import FusedRollout  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = single.DEV
_NAN = float("nan")
# every forward and backward instantiation, B = 1, B > 16 (grid x > 1 together with grid y > 1), gaps in weight rows, hist_gap
KERNEL_CASES = [c for c in hc.HORIZON_CASES if c.id in ("min", "nout16", "FD65", "FD161", "max", "S64-Wn0", "ref")]
assert len(KERNEL_CASES) == 7
assert {k for c in KERNEL_CASES for k in hc.expected_kernels(c)} == hc.ALL_KERNELS
HISTORIES = ("state_hist", "h1_hist", "h2_hist", "logits_hist", "orders_hist")
DZ = ("dz1_hist", "dz2_hist", "dz3_hist")
WEIGHTS = ("W1", "W2", "W3", "b2", "b3")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Slices:
    """K models' copies of one buffer, model m's slice m x stride floats behind model 0's, stride = slice + gap, NaN everywhere a
    kernel must not write: the gap, and inside a slice whatever lies outside (row < rows, t < T, b < B) - the row-stride gap, the
    padding columns."""

    def __init__(self, K, rows, T, ldb, hs, B, slice_floats, gap):
        assert rows * hs == slice_floats, (rows, hs, slice_floats)
        self.K, self.rows, self.T, self.ldb, self.hs, self.B = K, rows, T, ldb, hs, B
        self.stride = slice_floats + gap
        self.buf = torch.full((K * self.stride,), _NAN, device=DEV)

    def live(self, m):
        s = self.buf[m * self.stride:m * self.stride + self.rows * self.hs].view(self.rows, self.hs)
        return s[:, :self.T * self.ldb].view(self.rows, self.T, self.ldb)[:, :, :self.B]

    def outside_untouched(self):
        rest = self.buf.clone()
        keep, self.buf = self.buf, rest
        for m in range(self.K):
            self.live(m)[:] = _NAN
        self.buf = keep
        return _bits_equal(rest, torch.full_like(rest, _NAN))

    def all_untouched(self):
        return _bits_equal(self.buf, torch.full_like(self.buf, _NAN))


def _model_weights(c, m):
    """model 0: the case's weights and z1_obs; models 1, 2: redrawn from another generator seed (every tensor with the spread of the
    case's own, the first layer's per state row), the NaN gap columns of the weight rows kept"""
    k = hc.make_inputs(c)
    out = {n: k[n].clone() for n in WEIGHTS + ("z1_obs",)}
    if m == 0:
        return out
    FD, _, _ = hc.dims_of(c)
    gen = torch.Generator().manual_seed(7000 + 10 * c.seed + m)
    for n, cols in (("W1", FD), ("W2", c.H1), ("W3", c.H2)):
        live = k[n][:, :cols]
        spread = live.abs().mean(dim=0, keepdim=True) if n == "W1" else live.abs().mean()
        out[n][:, :cols] = torch.randn(live.shape, generator=gen) * spread * 1.25
    for n in ("b2", "b3"):
        out[n] = torch.randn(k[n].shape, generator=gen) * k[n].abs().mean() * 1.25
    out["z1_obs"] = torch.randn(k["z1_obs"].shape, generator=gen) * 0.5
    return out


def _single_run(c, w, with_backward=True):
    """one single-model launch pair on the case's inputs with the weights `w`: every output as CPU tensors"""
    L = single.prepare(c)
    for lin, (wn, bn) in zip(L.lin, (("W1", None), ("W2", "b2"), ("W3", "b3"))):
        lin.weight.copy_(w[wn].to(DEV))
        if bn:
            lin.bias.copy_(w[bn].to(DEV))
    L.z1_obs.live()[:] = w["z1_obs"].to(DEV)
    assert single.forward(L, with_hist=True) == hc.expected_kernels(c)[0]
    got = dict(rewards=L.rewards.live().cpu(), state_final=L.state_final.live().cpu(), **{n: h.live().cpu() for n, h in L.hist.items()})
    if with_backward:
        assert single.backward(L) == hc.expected_kernels(c)[1]
        got.update({n: h.live().cpu() for n, h in L.dz.items()})
    return got


_SINGLE = {}


def _reference(c, m):
    """computed once per (case, model), shared by the tests, never modified"""
    if (c.id, m) not in _SINGLE:
        _SINGLE[c.id, m] = _single_run(c, _model_weights(c, m))
    return _SINGLE[c.id, m]


class _Launch:
    """descriptor, strides and buffers of a K-model launch of case `c`"""

    def __init__(self, c, K):
        self.c, self.K = c, K
        self.L = L = single.prepare(c)   # shared inputs: state0, demand, mask, tables, g_reward (and the descriptor to start from)
        FD, n_out, n_ord = hc.dims_of(c)
        B, T, ld, hs = c.B, c.T, c.ldb, L.hs
        sl = self.slices = hz.ensemble_slices(L.desc)
        gaps = iter([4, 5, 6, 7, 8] + [4, 8] * 6)   # 4 - 8 floats over every slice (weights are read as scalars: any gap)
        # weights: one buffer per pointer of the descriptor, model m's copy at m x stride
        self.w, self.strides = {}, {}
        ws = [_model_weights(c, m) for m in range(K)]
        for n in WEIGHTS:
            stride = sl[n] + next(gaps)
            buf = torch.full((K * stride,), _NAN, device=DEV)
            for m in range(K):
                flat = ws[m][n].reshape(-1)
                assert flat.numel() == sl[n]
                buf[m * stride:m * stride + sl[n]] = flat.to(DEV)
            self.w[n], self.strides[n] = buf, stride
        S = lambda name, rows, T_=T, hs_=hs: _Slices(K, rows, T_, ld, hs_, B, sl[name], next(gaps))   # noqa: E731
        self.z1_obs = S("z1_obs", c.H1)
        for m in range(K):
            self.z1_obs.live(m)[:] = ws[m]["z1_obs"].to(DEV)
        self.rewards = S("rewards", 1, T, T * ld)
        self.state_final = S("state_final", FD, 1, ld)
        self.hist = dict(state_hist=S("state_hist", FD), h1_hist=S("h1_hist", c.H1), h2_hist=S("h2_hist", c.H2),
                         logits_hist=S("logits_hist", n_out), orders_hist=S("orders_hist", n_ord + c.Wn))
        self.dz = dict(dz1_hist=S("dz1", c.H1), dz2_hist=S("dz2", c.H2), dz3_hist=S("dz3", n_out))
        self.outputs = dict(rewards=self.rewards, state_final=self.state_final, **self.hist, **self.dz)
        for n, b in dict(z1_obs=self.z1_obs, rewards=self.rewards, state_final=self.state_final, **self.hist).items():
            self.strides[n] = b.stride
        for n, b in self.dz.items():
            self.strides[n[:3]] = b.stride
        assert all(4 <= self.strides[n] - sl[n] <= 8 for n in sl)
        d = self.desc = L.desc
        for n in WEIGHTS:
            setattr(d, n, self.w[n].data_ptr())
        self.ens = hz.ensemble_strides(K, **self.strides)

    def forward(self, with_hist=True, with_final=True):
        h = [self.hist[n].buf for n in HISTORIES] if with_hist else [None] * 5
        hz.horizon_ensemble_fwd(self.desc, self.ens, self.z1_obs.buf, self.L.state0, self.rewards.buf,
                                self.state_final.buf if with_final else None, *h)
        torch.cuda.synchronize()
        return _lib.lib().nic_last_kernel().decode()

    def backward(self):
        hz.horizon_ensemble_bwd(self.desc, self.ens, *(self.hist[n].buf for n in HISTORIES), self.L.g_reward, *(self.dz[n].buf for n in DZ))
        torch.cuda.synchronize()
        return _lib.lib().nic_last_kernel().decode()

    def inputs_unchanged(self, ws=None):
        ws = ws or [_model_weights(self.c, m) for m in range(self.K)]
        for n in WEIGHTS:
            rest = self.w[n].clone()
            for m in range(self.K):
                lo = m * self.strides[n]
                if not _bits_equal(rest[lo:lo + self.slices[n]], ws[m][n].reshape(-1).to(DEV)):
                    return False
                rest[lo:lo + self.slices[n]] = _NAN
            if not _bits_equal(rest, torch.full_like(rest, _NAN)):
                return False
        return self.z1_obs.outside_untouched()


def _ensemble_names(c, K):
    return tuple(n[:-1] + f",models={K}>" for n in hc.expected_kernels(c))


@pytest.mark.parametrize("K", [3, 1])
@pytest.mark.parametrize("c", KERNEL_CASES, ids=[c.id for c in KERNEL_CASES])
def test_ensemble_launch_is_k_single_model_launches(c, K):
    want_fwd, want_bwd = _ensemble_names(c, K)
    E = _Launch(c, K)
    assert E.forward() == want_fwd
    assert E.backward() == want_bwd
    for m in range(K):
        ref = _reference(c, m)
        for n, b in E.outputs.items():
            got = b.live(m).cpu()
            got = got[0] if n == "rewards" else got
            want = ref[n][0] if n == "rewards" else ref[n]
            assert not bool(torch.isnan(got).any()), (c.id, m, n)
            assert torch.equal(got.reshape(want.shape), want), (c.id, m, n)
    for n, b in E.outputs.items():
        assert b.outside_untouched(), (c.id, n, "written outside a model's (row < rows, t < T, b < B)")
    assert E.inputs_unchanged()
    if K > 1:   # the models do differ: equal outputs are not one model's copied K times
        assert not torch.equal(_reference(c, 0)["rewards"], _reference(c, 1)["rewards"])
        assert not torch.equal(_reference(c, 1)["dz1_hist"], _reference(c, 2)["dz1_hist"])


@pytest.mark.parametrize("id", ["ref", "FD65", "min"])
def test_ensemble_forward_without_histories(id):
    c = single._case(id)
    E = _Launch(c, 3)
    assert E.forward(with_hist=False) == _ensemble_names(c, 3)[0]
    for m in range(3):
        ref = _reference(c, m)
        assert torch.equal(E.rewards.live(m).cpu(), ref["rewards"]) and torch.equal(E.state_final.live(m).cpu(), ref["state_final"])
    assert E.rewards.outside_untouched() and E.state_final.outside_untouched()
    assert all(h.all_untouched() for h in E.hist.values())
    # ... and without the final state
    E.rewards.buf.fill_(_NAN)
    E.state_final.buf.fill_(_NAN)
    assert E.forward(with_hist=False, with_final=False) == _ensemble_names(c, 3)[0]
    for m in range(3):
        assert torch.equal(E.rewards.live(m).cpu(), _reference(c, m)["rewards"])
    assert E.rewards.outside_untouched() and E.state_final.all_untouched()
    assert all(h.all_untouched() for h in E.hist.values())


def test_ensemble_launchers_refuse_and_launch_nothing():
    lib, p = _lib.lib(), _lib.ptr
    c = single._case("ref")
    E = _Launch(c, 3)

    def fwd(desc, ens):
        return lib.nic_horizon_rollout_ensemble_fwd(desc, ens, p(E.z1_obs.buf), p(E.L.state0), p(E.rewards.buf), p(E.state_final.buf),
                                                    *(p(E.hist[n].buf) for n in HISTORIES), None)

    def bwd(desc, ens):
        return lib.nic_horizon_rollout_ensemble_bwd(desc, ens, *(p(E.hist[n].buf) for n in HISTORIES), E.L.g_reward.t2(),
                                                    *(p(E.dz[n].buf) for n in DZ), None)

    def refused(status, word):
        torch.cuda.synchronize()
        msg = lib.nic_last_error().decode()
        assert status != 0 and word in msg, (word, msg)
        assert all(b.all_untouched() for b in E.outputs.values()), word

    short = {"W1": "W1 stride shorter", "b3": "b3 stride shorter", "z1_obs": "z1_obs stride shorter", "rewards": "rewards stride shorter",
             "state_final": "final-state stride shorter", "state_hist": "state-history stride shorter",
             "orders_hist": "orders-history stride shorter"}
    for name, word in short.items():   # a stride below its slice
        refused(fwd(E.desc, hz.ensemble_strides(3, **{**E.strides, name: E.slices[name] - 4})), word)
    for name, word in (("h2_hist", "h2-history stride shorter"), ("dz1", "dz1 stride shorter"), ("dz3", "dz3 stride shorter")):
        refused(bwd(E.desc, hz.ensemble_strides(3, **{**E.strides, name: E.slices[name] - 4})), word)
    refused(fwd(E.desc, hz.ensemble_strides(3, **{**E.strides, "logits_hist": -E.strides["logits_hist"]})), "negative stride")
    refused(fwd(E.desc, hz.ensemble_strides(3, **{**E.strides, "h1_hist": E.strides["h1_hist"] + 2})), "multiples of 4 floats")
    for n_models in (0, 65536):
        refused(fwd(E.desc, hz.ensemble_strides(n_models, **E.strides)), "n_models must be 1..65535")
        refused(bwd(E.desc, hz.ensemble_strides(n_models, **E.strides)), "n_models must be 1..65535")
    assert fwd(E.desc, None) != 0 and "null ensemble" in lib.nic_last_error().decode()
    # round_orders: the forward takes it (evaluation), the backward does not
    E.desc.round_orders = 1
    refused(bwd(E.desc, E.ens), "rounded orders have no gradient")
    E.desc.round_orders = 0
    # a tape-mode descriptor (valid for the single-model launchers) has no ensemble form
    for id in ("levels-S5", "orders-S7"):
        T_ = single.prepare(single._case(id))
        assert lib.nic_horizon_rollout_ok(T_.desc) == 1
        one = hz.ensemble_strides(1, **{n: 1 << 24 for n in hz.ENSEMBLE_BUFFERS})
        st = lib.nic_horizon_rollout_ensemble_fwd(T_.desc, one, None, p(T_.state0), p(T_.rewards.buf), p(T_.state_final.buf),
                                                  p(T_.hist["state_hist"].buf), None, None, None, p(T_.hist["orders_hist"].buf), None)
        torch.cuda.synchronize()
        assert st != 0 and "only head_mode 0" in lib.nic_last_error().decode(), lib.nic_last_error()
        assert bool(torch.isnan(T_.rewards.buf).all()) and bool(torch.isnan(T_.hist["orders_hist"].buf).all())
    # after all that the same buffers still take a good request
    assert E.forward() == _ensemble_names(c, 3)[0]
    assert torch.equal(E.rewards.live(2).cpu(), _reference(c, 2)["rewards"])


# ---- engine ---------------------------------------------------------------------------------------------------------------------
ENGINE_CASES = ["f4_real_many_warehouses_data_driven", "f4_real_one_store_data_driven", "f4_real_one_store_read_files_data_driven"]
K_ENGINE = 3


def _models(g, c, k=K_ENGINE, hidden=None):
    """model 0: the fixture's weights; the others: the same architecture from other seeds"""
    F = g.params["net.master.0.weight"].shape[1]
    if hidden is not None:
        c["nn_params"]["neurons_per_hidden_layer"]["master"] = hidden
    out = []
    for i in range(k):
        torch.manual_seed(500 + i)
        m = tgr._model(g, c)
        eng = FusedRollout(m, c["problem_params"], DEV)
        eng.materialize(F)
        if i == 0 and hidden is None:
            tgr._load(m, g)
        out.append(m)
    return out


def _single_steps(models, c, data, train=True, discrete=False, periods=None):
    """K `FusedRollout.run` calls on the whole-horizon route: per model (total, reported, rewards [T][B], final state, gradients)"""
    out = []
    for m in models:
        eng = FusedRollout(m, c["problem_params"], DEV)
        for p_ in m.parameters():
            p_.grad = None
        tot, rep = eng.run(data, periods or c["periods"], c["ignore"], train=train, observation_params=c["observation_params"],
                           discrete_allocation=discrete)
        torch.cuda.synchronize()
        assert eng.horizon is not None
        out.append((float(tot), float(rep), eng.per_period_rewards().clone(), {k: v.clone() for k, v in eng.final_state().items()},
                    [p_.grad.clone() for p_ in m.parameters()] if train else None))
        for p_ in m.parameters():
            p_.grad = None
    return out


def _close(a, b):
    return abs(a - b) <= 1e-5 * abs(b)


def _check(ens, models, tt, want, train=True):
    total, reported = tt
    assert total.shape == reported.shape == (len(models),)
    rewards = ens.per_period_rewards()
    for m, (model, (tot, rep, rew, final, grads)) in enumerate(zip(models, want)):
        assert torch.equal(rewards[m], rew), m
        assert _close(float(total[m]), tot) and _close(float(reported[m]), rep), (m, float(total[m]), tot, float(reported[m]), rep)
        got_final = ens.final_state(m)
        assert set(got_final) == set(final)
        for k, v in final.items():
            assert torch.equal(got_final[k], v), (m, k)
        if train:
            for p_, gr in zip(model.parameters(), grads):
                assert p_.grad is not None and torch.equal(p_.grad, gr), m


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engine_matches_k_single_model_steps(name):
    g = Golden(name)
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    models = _models(g, c)
    want = _single_steps(models, c, data)
    assert want[0][0] != want[1][0] != want[2][0]
    ens = HorizonPolicyEnsemble(models, c["problem_params"], DEV)
    # evaluation first: no histories are taken
    ev = ens.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"])
    torch.cuda.synchronize()
    assert ens.hist is None and ens.grad is None and all(p_.grad is None for m in models for p_ in m.parameters())
    _check(ens, models, ev, want, train=False)
    tt = ens.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"])
    torch.cuda.synchronize()
    _check(ens, models, tt, want)
    assert torch.equal(tt[0], ev[0]) and torch.equal(tt[1], ev[1])   # the same reduction: the very bits
    assert ens.last_kernels["fwd"].endswith(",models=3>") and ens.last_kernels["bwd"].endswith(",models=3>")
    assert ens.weights.shape == (3, sum(p_.numel() for lin in models[0].master_linears() for p_ in (lin.weight, lin.bias)))
    for m, model in enumerate(models):   # gradients are views of one [K][P] buffer, in nn.Linear's own order
        flat = torch.cat([p_.grad.reshape(-1) for lin in model.master_linears() for p_ in (lin.weight, lin.bias)])
        assert torch.equal(ens.grad[m], flat)
        assert all(p_.grad.data_ptr() >= ens.grad.data_ptr() and p_.grad._base is not None for p_ in model.parameters())
    # discrete allocation: evaluation only
    with pytest.raises(ValueError, match="evaluation-time option"):
        ens.run(data, c["periods"], c["ignore"], train=True, observation_params=c["observation_params"], discrete_allocation=True)
    want_d = _single_steps(models, c, data, train=False, discrete=True)
    dd = ens.run(data, c["periods"], c["ignore"], train=False, observation_params=c["observation_params"], discrete_allocation=True)
    torch.cuda.synchronize()
    _check(ens, models, dd, want_d, train=False)
    assert any(not torch.equal(a[2], b[2]) for a, b in zip(want, want_d))   # (rounding does change the costs)


def test_engine_accumulates_reruns_and_takes_another_shape():
    g = Golden(ENGINE_CASES[0])
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    data2 = dict(data)
    data2["demands"] = (data["demands"] * 1.2 + 0.5).contiguous()
    half = {k: v[:5].contiguous() for k, v in data.items()}   # another batch size (B = 5: one workgroup, 11 idle lanes)
    models = _models(g, c)
    want, want2, want_half = _single_steps(models, c, data), _single_steps(models, c, data2), _single_steps(models, c, half)
    want_short = _single_steps(models, c, data, periods=c["periods"] - 3)
    ens = HorizonPolicyEnsemble(models, c["problem_params"], DEV)
    run = lambda d, **kw: ens.run(d, kw.pop("periods", c["periods"]), c["ignore"], observation_params=c["observation_params"], **kw)  # noqa: E731
    # accumulate_grads adds to a gradient that is already there
    for m in models:
        for p_ in m.parameters():
            p_.grad = torch.ones_like(p_)
    run(data, accumulate_grads=True)
    torch.cuda.synchronize()
    for model, w in zip(models, want):
        for p_, gr in zip(model.parameters(), w[4]):
            assert torch.equal(p_.grad, torch.ones_like(gr) + gr)
            p_.grad = None
    # the batch contents change, and change back; then other shapes on the same engine, and back
    for d, w, kw in ((data, want, {}), (data2, want2, {}), (data, want, {}), (half, want_half, {}),
                     (data, want_short, dict(periods=c["periods"] - 3)), (data, want, {})):
        tt = run(d, **kw)
        torch.cuda.synchronize()
        _check(ens, models, tt, w)
    assert want[0][0] != want2[0][0]


def test_engine_refuses_mixed_architectures_and_settings_it_does_not_take():
    g = Golden(ENGINE_CASES[0])
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    good = _models(g, c, k=2)
    other = _models(g, g.fresh_config(), k=1, hidden=[32, 16])
    with pytest.raises(ValueError, match=r"model 2: layer sizes \[32, 16, 66\] differ from model 0's \[32, 32, 66\]"):
        HorizonPolicyEnsemble(good + other, c["problem_params"], DEV)
    three = _models(g, g.fresh_config(), k=1, hidden=[32, 32, 32])   # FusedRollout takes it per period; the whole-horizon kernels do not
    ens = HorizonPolicyEnsemble(three, c["problem_params"], DEV)
    with pytest.raises(ValueError, match="whole-horizon kernels do not take this setting / policy"):
        ens.run(data, c["periods"], c["ignore"], observation_params=c["observation_params"])
    ens = HorizonPolicyEnsemble(good, c["problem_params"], DEV)
    obs = c["observation_params"].copy()
    obs["time_features"] = None
    with pytest.raises(ValueError, match="past-demand window"):
        ens.run(data, c["periods"], c["ignore"], observation_params=obs)


def test_models_of_an_ensemble_train_independently():
    """five steps of three torch.optim.Adam on the ensemble's gradients = the same five steps on three separate FusedRollout loops"""
    g = Golden(ENGINE_CASES[0])
    c = g.fresh_config()
    data = {k: v.to(DEV) for k, v in g.data.items()}
    lrs = (1e-3, 3e-3, 1e-2)
    a, b = _models(g, c), _models(g, g.fresh_config())
    for x, y in zip(a, b):
        assert all(torch.equal(p_, q_) for p_, q_ in zip(x.parameters(), y.parameters()))
    opts = [torch.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(a, lrs)]
    ens = HorizonPolicyEnsemble(a, c["problem_params"], DEV)
    for _ in range(5):
        ens.run(data, c["periods"], c["ignore"], observation_params=c["observation_params"])
        for o in opts:
            o.step()
    for m, lr in zip(b, lrs):
        eng, opt = FusedRollout(m, c["problem_params"], DEV), torch.optim.Adam(m.parameters(), lr=lr)
        for _ in range(5):
            eng.run(data, c["periods"], c["ignore"], observation_params=c["observation_params"])
            assert eng.horizon is not None
            opt.step()
    torch.cuda.synchronize()
    for x, y, start in zip(a, b, _models(g, g.fresh_config())):
        for p_, q_, s_ in zip(x.parameters(), y.parameters(), start.parameters()):
            assert torch.equal(p_, q_) and not torch.equal(p_, s_)
